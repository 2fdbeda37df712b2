// pfmpe_detect.hip — the LED detector on the device: LEDDetector::findLeds
// (pf_mpe_lib/src/led_detector.cpp:46-215, "LD") for one ROI of an 8-bit image, behind pfmpe_find_leds.
//
// The reference is OpenCV 2.4 calls; each is restated (oracle/detect_oracle.cpp lists the semantics):
//   k_det_mask     threshold (TOZERO / BINARY_INV) + GaussianBlur (8-bit-fraction integer kernels,
//                  reflect-101 borders, (sum + 2^15) >> 16) -> "pixel is nonzero" mask, with the 1-pixel
//                  frame cvStartFindContours zeroes.  16x16 tiles: thresholded tile + halo, then the row
//                  pass, staged in LDS; exact integer arithmetic.
//   k_det_label    per 32x32 tile in LDS: each pixel's 8-neighbour bit mask (bit s = direction s of
//                  icvFetchContour's table) and a tile-local union-find (W, NW, N, NE; atomicMin links to the
//                  lower index); the label is the local root's image index
//   k_det_merge    the global union-find over the links that cross tile borders only (agent-scope loads
//                  in find: other blocks' links bypass the non-coherent L1)
//   k_det_roots    flatten; every root (= the component's raster-first pixel, where the reference's raster
//                  scan starts its outer border) takes a slot
//   k_det_trace    one wave per component (grid-stride over the slots): a 64x64 window of neighbour masks
//                  staged in LDS, then lane 0 runs icvFetchContour's border following over it,
//                  polygon moments / area / bounding box on the fly, the size-aspect-circularity filter,
//                  the centre + ROI offset as float, cvUndistortPoints (5 iterations, P = K)
// The host orders the accepted detections as findContours returns them (reverse discovery = descending
// root index) and returns image_points_ (undistorted px) plus the distorted centres.
//
// pfmpe_find_leds_multi runs the same stages over R ROIs of one image in one launch sequence (k_detm_*: flat
// grids over all ROIs' tiles, pixels and components, one descriptor per ROI); the stage bodies are shared.
// pfmpe_find_leds_streams runs that sequence over the images of several cameras: a descriptor carries its own K and
// the address of its ROI's top-left pixel, in its context's staged image or in the crops the batch uploads
// (pfmpe_detect_plan.hpp: only the ROIs' pixels of a host image cross the host link; k_detm_pull).
#include "pf_batch.hpp"
#include "pfmpe_ctx.hpp"
#include "pfmpe_detect_plan.hpp"

using namespace pfmpe;
using namespace pfmpe_impl;

namespace pfmpe {

constexpr int kDetTile = 16;
constexpr int kDetMaxRadius = 15;      // kernel size <= 31 (sigma <= 5)
constexpr int kDetMaxComponents = 8192;

struct DetArgs {
  int k[2 * kDetMaxRadius + 1];  // Gaussian taps, 8 fraction bits
  int radius;
  int thr, active;
  int img_w, img_h, pitch;
  int rx, ry, W, H;              // ROI
  double K[9], D[5];
  double min_area, max_area, max_whd, max_circ;
};

struct DetRecord {  // one component (slot)
  int root, keep;
  float dx, dy;     // distorted centre + ROI offset (cv::Point2f)
  double ux, uy;    // undistorted (double(float))
  double area;
};

// icvFetchContour's direction table: 0 +x, 1 (+x,-y), 2 -y, 3 (-x,-y), 4 -x, 5 (-x,+y), 6 +y, 7 (+x,+y)
__device__ __forceinline__ int dir_dx(int s) { return (s == 0 || s == 1 || s == 7) ? 1 : ((s >= 3 && s <= 5) ? -1 : 0); }
__device__ __forceinline__ int dir_dy(int s) { return (s >= 1 && s <= 3) ? -1 : (s >= 5 ? 1 : 0); }

__device__ __forceinline__ int refl101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - p - 2;
  return p;
}

// The stage bodies below are shared by the single-ROI kernels (k_det_*: `a` is the kernel argument) and their
// batched forms (k_detm_*: `a` is the ROI's descriptor in device memory, the buffers are that ROI's); `a` is
// wave-uniform either way.
// one 16 x 16 tile at (x0, y0) of the ROI; the whole block.  pix: the ROI's top-left pixel, rows `pitch` apart (in the
// image, or in a crop of it: a.rx / a.ry are only the offset added to the centres)
__device__ __forceinline__ void det_mask_tile(const DetArgs& a, const uint8_t* __restrict__ pix, const int pitch,
                                              uint8_t* __restrict__ mask, const int x0, const int y0) {
  constexpr int T = kDetTile, HW = T + 2 * kDetMaxRadius;
  __shared__ int tb[HW][HW];    // thresholded tile + halo (rows, cols)
  __shared__ int rowp[HW][T];   // row pass
  const int r = a.radius, n = 2 * r + 1, span = T + 2 * r;
  for (int i = threadIdx.x; i < span * span; i += blockDim.x) {
    const int ty = i / span, tx = i - ty * span;
    const int gy = refl101(y0 + ty - r, a.H), gx = refl101(x0 + tx - r, a.W);
    const int v = pix[(int64_t)gy * pitch + gx];
    tb[ty][tx] = a.active ? (v > a.thr ? v : 0) : (v > a.thr ? 0 : 255);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < span * T; i += blockDim.x) {
    const int ty = i / T, tx = i - ty * T;
    int s = 0;
    for (int q = 0; q < n; ++q) s += a.k[q] * tb[ty][tx + q];
    rowp[ty][tx] = s;
  }
  __syncthreads();
  const int tx = threadIdx.x % T, ty = threadIdx.x / T;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= a.W || y >= a.H) return;
  long long s = 0;
  for (int q = 0; q < n; ++q) s += (long long)a.k[q] * rowp[ty + q][tx];
  const long long v = (s + (1 << 15)) >> 16;
  const bool frame = x == 0 || y == 0 || x == a.W - 1 || y == a.H - 1;
  mask[(int64_t)y * a.W + x] = (v > 0 && !frame) ? 1 : 0;
}
__global__ __launch_bounds__(kDetTile* kDetTile) void k_det_mask(const DetArgs a, const uint8_t* __restrict__ img,
                                                                  uint8_t* __restrict__ mask) {
  det_mask_tile(a, img + (int64_t)a.ry * a.pitch + a.rx, a.pitch, mask, blockIdx.x * kDetTile, blockIdx.y * kDetTile);
}

// Labelling, tile-local first: a 32 x 32 tile (+1 halo) of the mask in LDS gives each pixel its 8-neighbour
// bit mask (bit s = direction s of icvFetchContour's table: 0 +x, 1 (+x,-y), 2 -y, 3 (-x,-y), 4 -x,
// 5 (-x,+y), 6 +y, 7 (+x,+y)) and an LDS union-find over the tile's own W / NW / N / NE links (atomicMin
// to the lower index: the local root is the component's raster-first pixel in the tile).  The global
// label is that root's image index; k_det_merge then unites only links that cross a tile border.
constexpr int kLT = 32;
__device__ __forceinline__ int lfind(const int* L, int i) {
  for (int p = L[i]; p != i; p = L[i]) i = p;
  return i;
}
constexpr int kLabelBlock = 1024;
// one 32 x 32 tile at (x0, y0) of the ROI; the whole block (kLabelBlock threads)
__device__ __forceinline__ void det_label_tile(const DetArgs& a, const uint8_t* __restrict__ mask,
                                               uint8_t* __restrict__ nbr, int* __restrict__ label, const int x0,
                                               const int y0) {
  __shared__ uint8_t m[kLT + 2][kLT + 2];
  __shared__ int L[kLT * kLT];
  {  // branch-free: clamped in-bounds addresses, all loads in flight, then the selects
    constexpr int kN = ((kLT + 2) * (kLT + 2) + kLabelBlock - 1) / kLabelBlock;
    uint32_t v[kN];
    bool in[kN];
#pragma unroll
    for (int q = 0; q < kN; ++q) {
      const int i = threadIdx.x + kLabelBlock * q;
      const int ty = i / (kLT + 2), tx = i - ty * (kLT + 2);
      const int gx = x0 + tx - 1, gy = y0 + ty - 1;
      in[q] = i < (kLT + 2) * (kLT + 2) && gx >= 0 && gy >= 0 && gx < a.W && gy < a.H;
      v[q] = mask[(int64_t)min(max(gy, 0), a.H - 1) * a.W + min(max(gx, 0), a.W - 1)];
    }
#pragma unroll
    for (int q = 0; q < kN; ++q) {
      const int i = threadIdx.x + kLabelBlock * q;
      if (i < (kLT + 2) * (kLT + 2)) m[i / (kLT + 2)][i % (kLT + 2)] = in[q] ? (uint8_t)v[q] : (uint8_t)0;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLT * kLT; i += blockDim.x) {
    const int ly = i / kLT, lx = i - ly * kLT;
    L[i] = m[ly + 1][lx + 1] ? i : -1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLT * kLT; i += blockDim.x) {
    const int ly = i / kLT, lx = i - ly * kLT;
    if (!m[ly + 1][lx + 1]) continue;
    const int nb[4][2] = {{-1, 0}, {-1, -1}, {0, -1}, {1, -1}};  // W, NW, N, NE
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nx = lx + nb[q][0], ny = ly + nb[q][1];
      if (nx < 0 || ny < 0 || nx >= kLT || !m[ny + 1][nx + 1]) continue;
      int u = i, v = ny * kLT + nx;
      for (;;) {  // LDS union-find: link the higher root to the lower index
        u = lfind(L, u);
        v = lfind(L, v);
        if (u == v) break;
        if (u < v) {
          const int t = u;
          u = v;
          v = t;
        }
        const int old = atomicMin(&L[u], v);
        if (old == u) break;
        u = old;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLT * kLT; i += blockDim.x) {
    const int ly = i / kLT, lx = i - ly * kLT;
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx >= a.W || gy >= a.H) continue;
    const int64_t g = (int64_t)gy * a.W + gx;
    if (!m[ly + 1][lx + 1]) {
      label[g] = -1;
      nbr[g] = 0;
      continue;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) bits |= m[ly + 1 + dir_dy(s)][lx + 1 + dir_dx(s)] ? 1u << s : 0u;
    nbr[g] = (uint8_t)bits;
    const int r = lfind(L, i);
    label[g] = (y0 + r / kLT) * a.W + (x0 + r % kLT);
  }
}
__global__ __launch_bounds__(kLabelBlock) void k_det_label(const DetArgs a, const uint8_t* __restrict__ mask,
                                                   uint8_t* __restrict__ nbr, int* __restrict__ label) {
  det_label_tile(a, mask, nbr, label, blockIdx.x * kLT, blockIdx.y * kLT);
}

__device__ __forceinline__ int ld_label(const int* L, int i) {
  return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int find_root(const int* L, int i) {
  for (int p = ld_label(L, i); p != i; p = ld_label(L, i)) i = p;
  return i;
}
__device__ __forceinline__ void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root(L, a);
    b = find_root(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);  // link the higher root to the lower index
    if (old == a) return;
    a = old;
  }
}

// the links that cross a tile border (the left column's W / NW, the top row's NW / N / NE)
__device__ __forceinline__ void det_merge_pixel(const DetArgs& a, const uint8_t* __restrict__ nbr,
                                                int* __restrict__ label, const int64_t i) {
  if (i >= (int64_t)a.W * a.H) return;
  const int W = a.W;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const bool left = (x % kLT) == 0, top = (y % kLT) == 0, right = (x % kLT) == kLT - 1;
  if (!left && !top && !right) return;
  const uint32_t b = nbr[i];
  if (!b) return;
  if (left && (b & (1u << 4))) unite(label, (int)i, (int)i - 1);
  if ((left || top) && (b & (1u << 3))) unite(label, (int)i, (int)i - W - 1);
  if (top && (b & (1u << 2))) unite(label, (int)i, (int)i - W);
  if ((top || right) && (b & (1u << 1))) unite(label, (int)i, (int)i - W + 1);
}
__global__ void k_det_merge(const DetArgs a, const uint8_t* __restrict__ nbr, int* __restrict__ label) {
  det_merge_pixel(a, nbr, label, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ void k_det_roots(const DetArgs a, const uint8_t* __restrict__ mask, int* __restrict__ label,
                            int* __restrict__ count, int* __restrict__ roots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.W * a.H || !mask[i]) return;
  int r = (int)i;
  for (int p = label[r]; p != r; p = label[r]) r = p;
  label[i] = r;
  if (r == (int)i) {
    const int s = atomicAdd(count, 1);
    if (s < kDetMaxComponents) roots[s] = (int)i;
  }
}

// One block (one wave) per component slot: the wave stages a 64 x 64 window of neighbour masks (rows
// y0 .. y0+63 from the root down, columns x0-31 .. x0+32) in LDS, then lane 0 follows the border there
// (a point outside the window falls back to the global masks).
constexpr int kWin = 64;
// the component whose raster-first pixel is `root`: its record goes to *dst; one wave, `win` its LDS window
__device__ __forceinline__ void det_trace_component(const DetArgs& a, const uint8_t* __restrict__ nbr, const int root,
                                                    uint8_t (*win)[kWin], DetRecord* __restrict__ dst) {
  __syncthreads();  // the previous component's window reads are done
  const int W = a.W;
  const int x0 = root % W, y0 = root / W;
  const int wx = x0 - kWin / 2 + 1, wy = y0;
  {  // branch-free: every lane loads from a clamped in-bounds address, 16 loads in flight per batch
    const int lane = threadIdx.x;
    const int gx = wx + lane;
    const bool xin = gx >= 0 && gx < W;
    const int cx = min(max(gx, 0), W - 1);
    for (int r0 = 0; r0 < kWin; r0 += 16) {
      uint32_t v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = nbr[(int64_t)min(wy + r0 + q, a.H - 1) * W + cx];
#pragma unroll
      for (int q = 0; q < 16; ++q) win[r0 + q][lane] = (xin && wy + r0 + q < a.H) ? (uint8_t)v[q] : (uint8_t)0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
  auto nb = [&](int x, int y) -> uint32_t {
    const int lx = x - wx, ly = y - wy;
    if ((unsigned)lx < (unsigned)kWin && (unsigned)ly < (unsigned)kWin) return win[ly][lx];
    return nbr[(int64_t)y * W + x];
  };
  // icvFetchContour (CHAIN_APPROX_NONE), the contour points streamed into the polygon sums
  // The reference sums these in double; every term is an integer far below 2^53, so int64 sums are the
  // same numbers (exact either way) with a shorter dependency chain.
  int64_t a00 = 0, a10 = 0, a01 = 0, area2 = 0;
  int minx = x0, maxx = x0, miny = y0, maxy = y0;
  int64_t fx_ = 0, fy_ = 0, px_ = 0, py_ = 0;  // first point, previous point
  int np = 0;
  auto add_point = [&](int x, int y) {
    const int64_t xi = x, yi = y;
    if (np == 0) {
      fx_ = xi;
      fy_ = yi;
    } else {
      const int64_t dxy = px_ * yi - xi * py_;
      a00 += dxy;
      a10 += dxy * (px_ + xi);
      a01 += dxy * (py_ + yi);
      area2 += px_ * yi - py_ * xi;
    }
    px_ = xi;
    py_ = yi;
    minx = min(minx, x);
    maxx = max(maxx, x);
    miny = min(miny, y);
    maxy = max(maxy, y);
    ++np;
  };
  const uint32_t b0 = nb(x0, y0);
  int s = 4;
  do {
    s = (s - 1) & 7;
  } while (!((b0 >> s) & 1u) && s != 4);
  if (s == 4) {
    add_point(x0, y0);  // single-pixel domain
  } else {
    const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
    int x3 = x0, y3 = y0, px = x0, py = y0;
    for (int64_t guard = 0; guard < 4 * (int64_t)a.W * a.H + 8; ++guard) {
      const uint32_t bb = nb(x3, y3);
      const uint32_t rot = ((bb | (bb << 8)) >> ((s + 1) & 7)) & 0xffu;  // directions s+1, s+2, ... (cyclic)
      s = (s + 1 + __builtin_ctz(rot)) & 7;                            // first set (one exists)
      const int x4 = x3 + dir_dx(s), y4 = y3 + dir_dy(s);
      add_point(px, py);
      px += dir_dx(s);
      py += dir_dy(s);
      if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
      x3 = x4;
      y3 = y4;
      s = (s + 4) & 7;
    }
  }
  // closing edge last -> first (the reference's loop starts from the last point; the sums are the
  // same terms in a rotated order: exact for these integer-valued products)
  if (np > 1) {
    const int64_t xi = fx_, yi = fy_;
    const int64_t dxy = px_ * yi - xi * py_;
    a00 += dxy;
    a10 += dxy * (px_ + xi);
    a01 += dxy * (py_ + yi);
    area2 += px_ * yi - py_ * xi;
  }
  double m00 = 0, m10 = 0, m01 = 0;
  if (a00 != 0) {  // |a00| > FLT_EPSILON for an integer
    const double s2 = a00 > 0 ? 0.5 : -0.5, s6 = a00 > 0 ? 1.0 / 6 : -1.0 / 6;
    m00 = (double)a00 * s2;
    m10 = (double)a10 * s6;
    m01 = (double)a01 * s6;
  }
  const double area = fabs((double)area2 * 0.5);
  const int rw = maxx - minx + 1, rh = maxy - miny + 1;
  const double pi = 3.1415926535897932384626433832795;
  const double hw = (double)(rw / 2), hh = (double)(rh / 2);  // the reference's integer rect.width / 2
  const bool keep = area >= a.min_area && area <= a.max_area &&
                    fabs(1 - fmin((double)rw / (double)rh, (double)rh / (double)rw)) <= a.max_whd &&
                    fabs(1 - (area / (pi * (hw * hw)))) <= a.max_circ && fabs(1 - (area / (pi * (hh * hh)))) <= a.max_circ;
  DetRecord o{};
  o.root = root;
  o.keep = keep ? 1 : 0;
  o.area = area;
  if (keep) {
    const float mcx = (float)(m10 / m00) + (float)a.rx;
    const float mcy = (float)(m01 / m00) + (float)a.ry;
    o.dx = mcx;
    o.dy = mcy;
    const double* K = a.K;
    const double* D = a.D;
    const double ifx = 1. / K[0], ify = 1. / K[4];
    double x = ((double)mcx - K[2]) * ifx, y = ((double)mcy - K[5]) * ify;
    const double xs = x, ys = y;
    for (int j = 0; j < 5; ++j) {
      const double r2 = x * x + y * y;
      const double icdist = 1. / (1 + ((D[4] * r2 + D[1]) * r2 + D[0]) * r2);
      const double deltaX = 2 * D[2] * x * y + D[3] * (r2 + 2 * x * x);
      const double deltaY = D[2] * (r2 + 2 * y * y) + 2 * D[3] * x * y;
      x = (xs - deltaX) * icdist;
      y = (ys - deltaY) * icdist;
    }
    const double xx = K[0] * x + K[1] * y + K[2];
    const double yy = K[3] * x + K[4] * y + K[5];
    const double ww = 1. / (K[6] * x + K[7] * y + K[8]);
    o.ux = (double)(float)(xx * ww);
    o.uy = (double)(float)(yy * ww);
  }
  *dst = o;
  }  // lane 0
}
__global__ __launch_bounds__(64) void k_det_trace(const DetArgs a, const uint8_t* __restrict__ nbr,
                                                  const int* __restrict__ count, const int* __restrict__ roots,
                                                  DetRecord* __restrict__ rec) {
  __shared__ uint8_t win[kWin][kWin];
  const int nc = min(*count, kDetMaxComponents);
  for (int slot = blockIdx.x; slot < nc; slot += gridDim.x) det_trace_component(a, nbr, roots[slot], win, rec + slot);
}

// Output in findContours order (reverse discovery = descending root index), written straight into pinned
// host memory: rank of a kept record = number of kept records with a larger root.  One block.
struct DetOutHost {
  int32_t n, n_components, overflow, pad;
  double und[2 * kMaxBlobs];
  float dist[2 * kMaxBlobs];
};
constexpr int kEmitBlock = 1024;
// `total` components were counted, their records are rec[0 .. min(total, kDetMaxComponents)); the whole block
__device__ __forceinline__ void det_emit_block(const int total, const DetRecord* __restrict__ rec,
                                               DetOutHost* __restrict__ out) {
  __shared__ int kroot[kDetMaxComponents];
  __shared__ int nkept;
  const int nc = min(total, kDetMaxComponents);
  if (threadIdx.x == 0) nkept = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < nc; i += kEmitBlock)
    if (rec[i].keep) kroot[atomicAdd(&nkept, 1)] = i;  // slot ids, any order
  __syncthreads();
  const int nk = nkept;
  for (int t = threadIdx.x; t < nk; t += kEmitBlock) {
    const int i = kroot[t];
    const int r = rec[i].root;
    int rank = 0;
    for (int u = 0; u < nk; ++u) rank += rec[kroot[u]].root > r ? 1 : 0;
    if (rank < kMaxBlobs) {
      out->und[2 * rank] = rec[i].ux;
      out->und[2 * rank + 1] = rec[i].uy;
      out->dist[2 * rank] = rec[i].dx;
      out->dist[2 * rank + 1] = rec[i].dy;
    }
  }
  if (threadIdx.x == 0) {
    out->n = nk;
    out->n_components = total;
    out->overflow = total > kDetMaxComponents ? 1 : 0;
  }
}
__global__ __launch_bounds__(kEmitBlock) void k_det_emit(const int* __restrict__ count, const DetRecord* __restrict__ rec,
                                                         DetOutHost* __restrict__ out) {
  det_emit_block(*count, rec, out);
}

// ---------------------------------------------------------------------- R ROIs in one launch sequence
// pfmpe_find_leds_multi: the six stages over a batch of ROIs of one image.  Each ROI has a descriptor (DetDesc: its
// DetArgs and its own mask / nbr / label / roots / rec regions of the batch scratch, all in ROI-local pixel
// indexing, so labels and roots are the numbers the single call computes and the output order is its order).  The
// grids are flat: ROI r owns the blocks first[r] .. first[r + 1) of a stage (its 16 x 16 tiles, its 32 x 32 tiles,
// its 256-pixel ranges), so a small ROI next to a large one launches its own tile count only.  A block finds its
// ROI by one wave-wide comparison against the prefix (batch_stream_of_block, pf_batch.hpp), which replaces a
// block -> ROI map and its upload.
constexpr int kDetMaxRois = PFMPE_DETECT_MAX_ROIS;
static_assert(kDetMaxRois <= kBatchMaxStreams, "DetBatch::first* are read by batch_stream_of_block");
struct DetBatch {  // head of the batch's device image, the descriptors follow
  int R, pad[3];
  int first16[kDetMaxRois], first32[kDetMaxRois], firstpix[kDetMaxRois];  // first block of ROI r per stage
};
struct DetDesc {
  DetArgs a;
  uint8_t* mask;
  uint8_t* nbr;
  int* label;
  int* roots;
  DetRecord* rec;
  const uint8_t* pix;        // the ROI's top-left pixel: in a staged image, or in the batch's uploaded crops
  int pix_pitch;             // row pitch there
  int tiles16_x, tiles32_x;  // tiles per tile row
  int pad;
};
// counters, zeroed per call: components per ROI, then the work list's length
constexpr int kDetWorkCount = kDetMaxRois;
constexpr size_t kDetCounterBytes = (kDetMaxRois + 1) * sizeof(int);

constexpr int kStageBlock = 1024;  // the batch's first launch (k_batch_stage: head, descriptors, counters to zero)
static_assert(kDetWorkCount + 1 <= kStageBlock, "k_batch_stage zeroes one counter per thread");

// The streams batch's crops (pfmpe_find_leds_streams) from the leader's host-mapped pinned buffer into the scratch:
// n 16-byte words, one load per lane, consecutive lanes consecutive words, blocks grid-striding (the grid is sized
// by n up to kPullMaxGrid).  The alternative, one async copy command, is kept behind kDiagDetCopy for the A/B.
constexpr int kPullBlock = 256;
constexpr int kPullMaxGrid = 2048;
__global__ __launch_bounds__(kPullBlock) void k_detm_pull(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          const int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kPullBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPullBlock)
    dst[i] = src[i];
}

__global__ __launch_bounds__(kDetTile* kDetTile) void k_detm_mask(const DetBatch* __restrict__ hd,
                                                                   const DetDesc* __restrict__ descs) {
  const int roi = batch_stream_of_block(hd->first16, hd->R, blockIdx.x);
  const DetDesc& d = descs[roi];
  const int t = blockIdx.x - hd->first16[roi];
  const int ty = t / d.tiles16_x, tx = t - ty * d.tiles16_x;
  det_mask_tile(d.a, d.pix, d.pix_pitch, d.mask, tx * kDetTile, ty * kDetTile);
}

__global__ __launch_bounds__(kLabelBlock) void k_detm_label(const DetBatch* __restrict__ hd,
                                                            const DetDesc* __restrict__ descs) {
  const int roi = batch_stream_of_block(hd->first32, hd->R, blockIdx.x);
  const DetDesc& d = descs[roi];
  const int t = blockIdx.x - hd->first32[roi];
  const int ty = t / d.tiles32_x, tx = t - ty * d.tiles32_x;
  det_label_tile(d.a, d.mask, d.nbr, d.label, tx * kLT, ty * kLT);
}

constexpr int kPixBlock = 256;  // an ROI's pixels are rounded up to whole blocks: a block belongs to one ROI
__global__ __launch_bounds__(kPixBlock) void k_detm_merge(const DetBatch* __restrict__ hd,
                                                          const DetDesc* __restrict__ descs) {
  const int roi = batch_stream_of_block(hd->firstpix, hd->R, blockIdx.x);
  const DetDesc& d = descs[roi];
  det_merge_pixel(d.a, d.nbr, d.label, (int64_t)(blockIdx.x - hd->firstpix[roi]) * kPixBlock + threadIdx.x);
}

// A root takes a slot of its ROI and, while the ROI has slots left, an entry (roi << 16 | slot) of the flat work list.
__global__ __launch_bounds__(kPixBlock) void k_detm_roots(const DetBatch* __restrict__ hd,
                                                          const DetDesc* __restrict__ descs, int* __restrict__ counters,
                                                          uint32_t* __restrict__ work) {
  const int roi = batch_stream_of_block(hd->firstpix, hd->R, blockIdx.x);
  const DetDesc& d = descs[roi];
  const int64_t i = (int64_t)(blockIdx.x - hd->firstpix[roi]) * kPixBlock + threadIdx.x;
  if (i >= (int64_t)d.a.W * d.a.H || !d.mask[i]) return;
  int* label = d.label;
  int r = (int)i;
  for (int p = label[r]; p != r; p = label[r]) r = p;
  label[i] = r;
  if (r == (int)i) {
    const int s = atomicAdd(counters + roi, 1);
    if (s < kDetMaxComponents) {
      d.roots[s] = (int)i;
      work[atomicAdd(counters + kDetWorkCount, 1)] = (uint32_t)roi << 16 | (uint32_t)s;
    }
  }
}

// Waves grid-stride over the work list, so they stay busy whatever the split of components between the ROIs.
__global__ __launch_bounds__(64) void k_detm_trace(const DetDesc* __restrict__ descs, const int* __restrict__ counters,
                                                   const uint32_t* __restrict__ work) {
  __shared__ uint8_t win[kWin][kWin];
  const int nw = counters[kDetWorkCount];  // <= R * kDetMaxComponents: only slots below the cap are listed
  for (int w = blockIdx.x; w < nw; w += gridDim.x) {
    const uint32_t e = __builtin_amdgcn_readfirstlane(work[w]);
    const DetDesc& d = descs[e >> 16];
    const int slot = (int)(e & 0xffffu);
    det_trace_component(d.a, d.nbr, d.roots[slot], win, d.rec + slot);
  }
}

// one block per ROI; out: R records in pinned host memory
__global__ __launch_bounds__(kEmitBlock) void k_detm_emit(const DetDesc* __restrict__ descs,
                                                          const int* __restrict__ counters,
                                                          DetOutHost* __restrict__ out) {
  det_emit_block(counters[blockIdx.x], descs[blockIdx.x].rec, out + blockIdx.x);
}

}  // namespace pfmpe

namespace {

// getGaussianKernel(n, sigma, CV_32F) -> 8-bit-fraction ints (the 8U separable path of OpenCV 2.4)
std::vector<int> gaussian_q8(int n, double sigma) {
  std::vector<float> cf(n);
  const double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
  const double scale2X = -0.5 / (sx * sx);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    cf[i] = (float)std::exp(scale2X * x * x);
    sum += cf[i];
  }
  sum = 1. / sum;
  std::vector<int> k(n);
  for (int i = 0; i < n; ++i) {
    cf[i] = (float)(cf[i] * sum);
    k[i] = (int)std::nearbyint((double)cf[i] * 256.0);
  }
  return k;
}

struct DetBuffers {
  uint8_t* mask;
  uint8_t* nbr;
  int* label;
  int* count;
  int* roots;
  DetRecord* rec;
};

int det_buffers(pfmpe_ctx* c, int64_t npix, DetBuffers& b) {
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_mask = 0, o_nbr = o_mask + al(npix), o_label = o_nbr + al(npix);
  const size_t o_count = o_label + al(npix * 4), o_roots = o_count + 256;
  const size_t o_rec = o_roots + al(kDetMaxComponents * 4), total = o_rec + al(kDetMaxComponents * sizeof(DetRecord));
  RET(c->d_det.grow(c, total, total));
  unsigned char* d = c->d_det.get();
  b = DetBuffers{d + o_mask, d + o_nbr, (int*)(d + o_label), (int*)(d + o_count), (int*)(d + o_roots),
                 (DetRecord*)(d + o_rec)};
  return PFMPE_OK;
}

// what is wrong with one ROI's parameters for a width x height image (nullptr: nothing)
const char* det_check(const pfmpe_detect_params* prm, int width, int height) {
  if (const char* why = pfmpe_plan::roi_geometry(prm, width, height)) return why;
  if (!(prm->gaussian_sigma > 0) || prm->gaussian_sigma > 5.0) return "gaussian_sigma must be in (0, 5]";
  return nullptr;
}

// the kernels' arguments for one ROI (checked by det_check)
DetArgs det_args(const pfmpe_ctx* c, const pfmpe_detect_params* prm, int width, int height, int pitch) {
  DetArgs a{};
  const int n = (int)std::nearbyint(prm->gaussian_sigma * 3 * 2 + 1) | 1;  // ksize from sigma for 8U (cvRound)
  const std::vector<int> k = gaussian_q8(n, prm->gaussian_sigma);
  for (int i = 0; i < n; ++i) a.k[i] = k[i];
  a.radius = n / 2;
  a.thr = prm->threshold_value;
  a.active = prm->active_markers ? 1 : 0;
  a.img_w = width;
  a.img_h = height;
  a.pitch = pitch;
  const pfmpe_plan::Rect roi = pfmpe_plan::rect_of(prm, width, height);
  a.rx = roi.x;
  a.ry = roi.y;
  a.W = roi.w;
  a.H = roi.h;
  std::memcpy(a.K, c->K, sizeof(a.K));
  std::memcpy(a.D, prm->D, sizeof(a.D));
  a.min_area = prm->min_blob_area;
  a.max_area = prm->max_blob_area;
  a.max_whd = prm->max_width_height_distortion;
  a.max_circ = prm->max_circular_distortion;
  return a;
}

// Batch scratch (pfmpe_find_leds_multi, pfmpe_find_leds_streams), one allocation: the counters, the batch head + R
// descriptors (the pinned image h_detm is uploaded there), the work list, the uploaded crops (crop_bytes), then per ROI
// mask | nbr | label | roots | rec, each 256-byte aligned.  Fills the descriptors' pointers.
constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr size_t kDetmHead = al256(kDetCounterBytes);
constexpr size_t kDetmDesc = kDetmHead + al256(sizeof(DetBatch));
int detm_buffers(pfmpe_ctx* c, int R, DetDesc* descs, size_t crop_bytes, size_t* o_work, size_t* o_crop) {
  *o_work = kDetmDesc + al256((size_t)R * sizeof(DetDesc));
  *o_crop = *o_work + al256((size_t)R * kDetMaxComponents * sizeof(uint32_t));  // the uploaded crops (streams batch)
  size_t total = *o_crop + al256(crop_bytes);
  std::vector<size_t> base(R);
  for (int r = 0; r < R; ++r) {
    const size_t npix = (size_t)descs[r].a.W * descs[r].a.H;
    base[r] = total;
    total += 2 * al256(npix) + al256(npix * 4) + al256(kDetMaxComponents * sizeof(int)) +
             al256(kDetMaxComponents * sizeof(DetRecord));
  }
  RET(c->d_detm.grow(c, total, total));
  for (int r = 0; r < R; ++r) {
    const size_t npix = (size_t)descs[r].a.W * descs[r].a.H;
    unsigned char* p = c->d_detm.get() + base[r];
    descs[r].mask = p;
    descs[r].nbr = (p += al256(npix));
    descs[r].label = (int*)(p += al256(npix));
    descs[r].roots = (int*)(p += al256(npix * 4));
    descs[r].rec = (DetRecord*)(p += al256(kDetMaxComponents * sizeof(int)));
  }
  return PFMPE_OK;
}

// one ROI's output record h (pinned, written by the emit kernel) -> the caller's arrays (max_out rows) and out
void det_take(const DetOutHost& h, double* blobs, float* distorted, int max_out, pfmpe_detect_out* out) {
  const int nw = std::min(std::min(h.n, max_out), kMaxBlobs);
  if (nw > 0) {
    std::memcpy(blobs, h.und, 2 * (size_t)nw * sizeof(double));
    if (distorted) std::memcpy(distorted, h.dist, 2 * (size_t)nw * sizeof(float));
  }
  out->n = h.n;
  out->n_components = h.n_components;
  out->overflow = h.overflow;
}

// A batch on its leader c (pfmpe_find_leds_multi, pfmpe_find_leds_streams), after every check: the pinned image of the
// batch head and the descriptors, the scratch, the launch sequence, one synchronise, the results.  fill(r, d) sets
// entry r's d.a and, for an entry that reads an image where it is, d.pix / d.pix_pitch.  An entry with
// crops[r].offset >= 0 (crops null: none) reads the batch's uploaded crops: pack(p) writes their upload_bytes into the
// leader's pinned buffer, which one more launch then moves into the scratch.
template <typename Fill, typename Pack>
int detm_run(pfmpe_ctx* c, int R, Fill&& fill, const pfmpe_detect_crop* crops, int64_t upload_bytes, Pack&& pack,
             double* blobs, float* distorted, int max_out, pfmpe_detect_out* out) {
  RET(c->h_detm.ensure(c, al256(sizeof(DetBatch)) + kDetMaxRois * sizeof(DetDesc)));
  RET(c->h_detm_out.grow(c, (size_t)R * sizeof(DetOutHost), (size_t)R * sizeof(DetOutHost)));
  if (upload_bytes > 0) RET(c->h_detm_pix.grow(c, (size_t)upload_bytes, (size_t)upload_bytes * 2));
  // the pinned image of the batch head and the descriptors, then one upload
  DetBatch* hd = (DetBatch*)c->h_detm.get();
  DetDesc* descs = (DetDesc*)(c->h_detm.get() + al256(sizeof(DetBatch)));
  std::memset(hd, 0, sizeof(*hd));
  hd->R = R;
  int n16 = 0, n32 = 0, npb = 0;
  for (int r = 0; r < R; ++r) {
    DetDesc& d = descs[r];
    fill(r, d);
    d.tiles16_x = (d.a.W + kDetTile - 1) / kDetTile;
    d.tiles32_x = (d.a.W + kLT - 1) / kLT;
    hd->first16[r] = n16;
    hd->first32[r] = n32;
    hd->firstpix[r] = npb;
    n16 += d.tiles16_x * ((d.a.H + kDetTile - 1) / kDetTile);
    n32 += d.tiles32_x * ((d.a.H + kLT - 1) / kLT);
    npb += (int)(((int64_t)d.a.W * d.a.H + kPixBlock - 1) / kPixBlock);
  }
  size_t o_work = 0, o_crop = 0;
  RET(detm_buffers(c, R, descs, (size_t)upload_bytes, &o_work, &o_crop));
  for (int r = 0; crops && r < R; ++r)
    if (crops[r].offset >= 0) {
      descs[r].pix = c->d_detm.get() + o_crop + crops[r].offset;
      descs[r].pix_pitch = crops[r].pitch;
    }
  if (upload_bytes > 0) pack(c->h_detm_pix.get());
  int* counters = (int*)c->d_detm.get();
  const DetBatch* dhd = (const DetBatch*)(c->d_detm.get() + kDetmHead);
  const DetDesc* ddescs = (const DetDesc*)(c->d_detm.get() + kDetmDesc);
  uint32_t* work = (uint32_t*)(c->d_detm.get() + o_work);
  static_assert(sizeof(DetDesc) % sizeof(uint64_t) == 0, "k_batch_stage copies 8-byte words");
  const int stage_words = (int)((al256(sizeof(DetBatch)) + (size_t)R * sizeof(DetDesc)) / sizeof(uint64_t));
  const uint64_t* stage_src = (const uint64_t*)c->h_detm.dev();
  DetOutHost* hout = (DetOutHost*)c->h_detm_out.get();
  DetOutHost* dout = (DetOutHost*)c->h_detm_out.dev();
  const int64_t pull_n = upload_bytes / (int64_t)sizeof(uint4);  // upload_bytes is a multiple of 256
  const unsigned pull_grid = (unsigned)std::min<int64_t>((pull_n + kPullBlock - 1) / kPullBlock, kPullMaxGrid);
  RET(timed(c, [&] {
    hipError_t copy_err = hipSuccess;
    int rc = launch(c, PFMPE_K_DETECT, [&] {
      hipLaunchKernelGGL((k_batch_stage<kStageBlock>), dim3(1), dim3(kStageBlock), 0, c->stream, stage_src,
                         (uint64_t*)(c->d_detm.get() + kDetmHead), stage_words, counters, kDetWorkCount + 1);
      if (pull_n > 0) {
        if (c->diag & kDiagDetCopy)
          copy_err = hipMemcpyAsync(c->d_detm.get() + o_crop, c->h_detm_pix.get(), (size_t)upload_bytes,
                                    hipMemcpyHostToDevice, c->stream);
        else
          hipLaunchKernelGGL(k_detm_pull, dim3(pull_grid), dim3(kPullBlock), 0, c->stream,
                             (const uint4*)c->h_detm_pix.dev(), (uint4*)(c->d_detm.get() + o_crop), pull_n);
      }
      hipLaunchKernelGGL(k_detm_mask, dim3(n16), dim3(kDetTile * kDetTile), 0, c->stream, dhd, ddescs);
      hipLaunchKernelGGL(k_detm_label, dim3(n32), dim3(kLabelBlock), 0, c->stream, dhd, ddescs);
      hipLaunchKernelGGL(k_detm_merge, dim3(npb), dim3(kPixBlock), 0, c->stream, dhd, ddescs);
      hipLaunchKernelGGL(k_detm_roots, dim3(npb), dim3(kPixBlock), 0, c->stream, dhd, ddescs, counters, work);
      hipLaunchKernelGGL(k_detm_trace, dim3(512), dim3(64), 0, c->stream, ddescs, (const int*)counters,
                         (const uint32_t*)work);
      hipLaunchKernelGGL(k_detm_emit, dim3(R), dim3(kEmitBlock), 0, c->stream, ddescs, (const int*)counters, dout);
    });
    // whatever was enqueued is drained before returning, so a failure leaves nothing of the batch pending
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (rc == PFMPE_OK && copy_err != hipSuccess)
      rc = fail(c, PFMPE_E_HIP, std::string("crop upload: ") + hipGetErrorString(copy_err));
    if (rc == PFMPE_OK && se != hipSuccess)
      rc = fail(c, PFMPE_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    if (rc == PFMPE_OK && c->timing_now) rc = harvest_timing(c);
    return rc;
  }));
  for (int r = 0; r < R; ++r)
    det_take(hout[r], blobs + (size_t)r * 2 * max_out, distorted ? distorted + (size_t)r * 2 * max_out : nullptr, max_out,
             &out[r]);
  return PFMPE_OK;
}

}  // namespace

extern "C" {

void pfmpe_default_detect_params(pfmpe_detect_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->threshold_value = 240;  // README.md:331-337 launch values
  p->active_markers = 1;
  p->gaussian_sigma = 0.6;
  p->min_blob_area = 20;
  p->max_blob_area = 160;
  p->max_width_height_distortion = 0.7;
  p->max_circular_distortion = 0.7;
  p->roi_w = -1;  // whole image
  p->roi_h = -1;
}

// PE:429-432 / PE:454-457: the width and height are clipped against the already moved x and y; 64-bit
// intermediates, so no margin overflows
int pfmpe_host_grow_roi(const int32_t roi[4], int32_t margin, int32_t image_w, int32_t image_h, int32_t grown[4]) {
  if (!roi || !grown || margin < 0 || image_w < 1 || image_h < 1) return PFMPE_E_ARG;
  const int64_t x = std::max<int64_t>((int64_t)roi[0] - margin, 0), y = std::max<int64_t>((int64_t)roi[1] - margin, 0);
  const int64_t w = std::min<int64_t>((int64_t)roi[2] + 2 * (int64_t)margin, (int64_t)image_w - x);
  const int64_t h = std::min<int64_t>((int64_t)roi[3] + 2 * (int64_t)margin, (int64_t)image_h - y);
  grown[0] = (int32_t)x;
  grown[1] = (int32_t)y;
  grown[2] = (int32_t)w;
  grown[3] = (int32_t)h;
  return PFMPE_OK;
}

int pfmpe_stage_image(pfmpe_ctx* c, const uint8_t* image, int width, int height, int pitch) {
  if (!c) return PFMPE_E_ARG;
  if (!image || width < 1 || height < 1 || pitch < width) return fail(c, PFMPE_E_ARG, "stage_image: bad image");
  RET(set_device(c));
  const size_t bytes = (size_t)pitch * height;
  RET(c->d_img.grow(c, bytes, bytes));
  HIPCHK(c, hipMemcpyAsync(c->d_img.get(), image, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->img_w = width;
  c->img_h = height;
  c->img_pitch = pitch;
  return PFMPE_OK;
}

int pfmpe_find_leds(pfmpe_ctx* c, const uint8_t* image, int width, int height, int pitch,
                    const pfmpe_detect_params* prm, double* blobs, float* distorted, int max_out,
                    pfmpe_detect_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!prm || !out || max_out < 0 || (max_out > 0 && !blobs)) return fail(c, PFMPE_E_ARG, "find_leds: bad arguments");
  if (!c->has_model) return fail(c, PFMPE_E_STATE, "find_leds: set_model first (K)");
  if (image) {
    RET(pfmpe_stage_image(c, image, width, height, pitch));
  } else if (!c->d_img || c->img_w != width || c->img_h != height || c->img_pitch != pitch) {
    return fail(c, PFMPE_E_STATE, "find_leds: no staged image of this size (pfmpe_stage_image)");
  }
  if (const char* why = det_check(prm, width, height)) return fail(c, PFMPE_E_ARG, std::string("find_leds: ") + why);
  RET(set_device(c));
  const DetArgs a = det_args(c, prm, width, height, pitch);
  const int W = a.W, H = a.H;
  const int64_t npix = (int64_t)W * H;
  DetBuffers b;
  RET(det_buffers(c, npix, b));
  HIPCHK(c, hipMemsetAsync(b.count, 0, sizeof(int), c->stream));
  const unsigned g1 = (unsigned)((npix + 255) / 256);
  RET(c->h_det.ensure(c, sizeof(DetOutHost)));
  DetOutHost* hout = (DetOutHost*)c->h_det.get();
  DetOutHost* dout = (DetOutHost*)c->h_det.dev();
  RET(timed(c, [&] {
    RET(launch(c, PFMPE_K_DETECT, [&] {
      hipLaunchKernelGGL(k_det_mask, dim3((W + kDetTile - 1) / kDetTile, (H + kDetTile - 1) / kDetTile),
                         dim3(kDetTile * kDetTile), 0, c->stream, a, c->d_img.get(), b.mask);
      hipLaunchKernelGGL(k_det_label, dim3((W + kLT - 1) / kLT, (H + kLT - 1) / kLT), dim3(kLabelBlock), 0, c->stream, a,
                         b.mask, b.nbr, b.label);
      hipLaunchKernelGGL(k_det_merge, dim3(g1), dim3(256), 0, c->stream, a, b.nbr, b.label);
      hipLaunchKernelGGL(k_det_roots, dim3(g1), dim3(256), 0, c->stream, a, b.mask, b.label, b.count, b.roots);
      hipLaunchKernelGGL(k_det_trace, dim3(512), dim3(64), 0, c->stream, a, b.nbr, b.count, b.roots, b.rec);
      hipLaunchKernelGGL(k_det_emit, dim3(1), dim3(kEmitBlock), 0, c->stream, b.count, b.rec, dout);
    }));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return c->timing_now ? harvest_timing(c) : (int)PFMPE_OK;
  }));
  det_take(*hout, blobs, distorted, max_out, out);
  return PFMPE_OK;
}

int pfmpe_find_leds_multi(pfmpe_ctx* c, const uint8_t* image, int width, int height, int pitch,
                          const pfmpe_detect_params* prm, int R, double* blobs, float* distorted, int max_out,
                          pfmpe_detect_out* out) {
  if (!c) return PFMPE_E_ARG;
  if (!prm || !out || R < 1 || max_out < 0 || (max_out > 0 && !blobs))
    return fail(c, PFMPE_E_ARG, "find_leds_multi: bad arguments");
  if (R > PFMPE_DETECT_MAX_ROIS) return fail(c, PFMPE_E_CAP, "find_leds_multi: R exceeds PFMPE_DETECT_MAX_ROIS");
  if (!c->has_model) return fail(c, PFMPE_E_STATE, "find_leds_multi: set_model first (K)");
  if (image) {
    if (width < 1 || height < 1 || pitch < width) return fail(c, PFMPE_E_ARG, "find_leds_multi: bad image");
  } else if (!c->d_img || c->img_w != width || c->img_h != height || c->img_pitch != pitch) {
    return fail(c, PFMPE_E_STATE, "find_leds_multi: no staged image of this size (pfmpe_stage_image)");
  }
  for (int r = 0; r < R; ++r)
    if (const char* why = det_check(prm + r, width, height))
      return fail(c, PFMPE_E_ARG, "find_leds_multi: roi " + std::to_string(r) + ": " + why);
  if (image) RET(pfmpe_stage_image(c, image, width, height, pitch));
  RET(set_device(c));
  return detm_run(
      c, R,
      [&](int r, DetDesc& d) {
        d.a = det_args(c, prm + r, width, height, pitch);
        d.pix = c->d_img.get() + (int64_t)d.a.ry * pitch + d.a.rx;
        d.pix_pitch = pitch;
      },
      nullptr, 0, [](uint8_t*) {}, blobs, distorted, max_out, out);
}

int pfmpe_find_leds_streams(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                            const pfmpe_detect_params* prm, int R, double* blobs, float* distorted, int max_out,
                            pfmpe_detect_out* out) {
  if (!images || I < 1 || !images[0].ctx) return PFMPE_E_ARG;
  pfmpe_ctx* c0 = images[0].ctx;
  const std::string who = "find_leds_streams: ";
  if (!out || max_out < 0 || (max_out > 0 && !blobs)) return fail(c0, PFMPE_E_ARG, who + "bad arguments");
  std::string why;
  if (const int rc = pfmpe_plan::check(images, I, image_of, prm, R, det_check, &why)) return fail(c0, rc, who + why);
  BatchMembers members("find_leds_streams", I);  // the batch's contexts, each once, the leader first
  for (int i = 0; i < I; ++i) {
    const pfmpe_detect_image& im = images[i];
    pfmpe_ctx* c = im.ctx;
    const std::string at = who + "image " + std::to_string(i) + ": ";
    if (!c) return fail(c0, PFMPE_E_ARG, at + "null context");
    if (c->device != c0->device) return fail(c0, PFMPE_E_ARG, at + "device must match images[0].ctx");
    if (!c->has_model) return fail(c0, PFMPE_E_STATE, at + "set_model first (K)");
    if (!im.image && (!c->d_img || c->img_w != im.width || c->img_h != im.height || c->img_pitch != im.pitch))
      return fail(c0, PFMPE_E_STATE, at + "no staged image of this size (pfmpe_stage_image)");
    members.add(c);
  }
  pfmpe_detect_crop crops[PFMPE_DETECT_MAX_ROIS];
  int64_t upload_bytes = 0;
  if (const int rc = pfmpe_plan::build(images, image_of, prm, R, crops, &upload_bytes))
    return fail(c0, rc, who + "the ROIs' pixels exceed the upload limit");
  RET(set_device(c0));
  // every member's staging before the batch; the call's end is detm_run's (shared with find_leds_multi), then commit()
  RET(members.order());
  RET(detm_run(
      c0, R,
      [&](int r, DetDesc& d) {
        const pfmpe_detect_image& im = images[image_of[r]];
        d.a = det_args(im.ctx, prm + r, im.width, im.height, im.pitch);
        if (!im.image) {
          d.pix = im.ctx->d_img.get() + (int64_t)d.a.ry * im.pitch + d.a.rx;
          d.pix_pitch = im.pitch;
        }
      },
      crops, upload_bytes, [&](uint8_t* p) { pfmpe_plan::pack(images, image_of, prm, R, crops, p, upload_bytes); },
      blobs, distorted, max_out, out));
  members.commit();  // nothing of the batch is pending: no member needs a fence
  return PFMPE_OK;
}

}  // extern "C"
