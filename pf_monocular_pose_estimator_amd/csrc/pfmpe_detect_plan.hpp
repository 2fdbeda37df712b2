#pragma once
// pfmpe_detect_plan.hpp — the upload plan of pfmpe_find_leds_streams, host C++ only (no device code, no HIP): which
// pixels of the batch's host images cross the host link, and where they land in the upload buffer.  Shared by the
// host-only entry points (pfmpe_detect_plan.cpp: pfmpe_host_detect_plan / pfmpe_host_detect_pack) and the device
// call (pfmpe_detect.hip), so the plan a test pins is the plan the batch runs.
//
// An entry's rectangle is its ROI in its image (a negative roi_w: the whole width, a negative roi_h: the whole
// height).  An entry on a staged image (image == NULL) uploads nothing.  An entry r on a host image is served by its
// owner: of the entries of the same image index whose rectangle contains r's (r included), the one with the largest
// area, the lowest index on a tie.  An owner is its own owner, so crops never chain.  Own crops lie in ascending
// entry index, each 256-byte aligned, rows padded to a multiple of 16 bytes; a shared entry points into its owner's
// crop (the retry on an enlarged ROI, PE:452-463, uploads nothing extra).
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/pfmpe.h"

namespace pfmpe_plan {

struct Rect {
  int x, y, w, h;
};
// the rectangle det_args derives (pfmpe_detect.hip)
inline Rect rect_of(const pfmpe_detect_params* p, int width, int height) {
  return Rect{p->roi_w < 0 ? 0 : p->roi_x, p->roi_h < 0 ? 0 : p->roi_y, p->roi_w < 0 ? width : p->roi_w,
              p->roi_h < 0 ? height : p->roi_h};
}
inline bool rect_inside_image(const Rect& r, int width, int height) {
  return r.x >= 0 && r.y >= 0 && r.w >= 1 && r.h >= 1 && (int64_t)r.x + r.w <= width && (int64_t)r.y + r.h <= height;
}
// what is wrong with one entry's rectangle (nullptr: nothing): the geometric part of the detector's parameter check
inline const char* roi_geometry(const pfmpe_detect_params* p, int width, int height) {
  return rect_inside_image(rect_of(p, width, height), width, height) ? nullptr : "ROI outside the image";
}
inline bool contains(const Rect& o, const Rect& r) {
  return o.x <= r.x && o.y <= r.y && o.x + o.w >= r.x + r.w && o.y + o.h >= r.y + r.h;
}
constexpr int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }
// uploads beyond this are refused (PFMPE_E_CAP): 64 crops of it still fit an int64 byte count
constexpr int64_t kMaxUploadBytes = (int64_t)1 << 40;

// The checks the plan, the pack and the device call share, in this order: pointers and counts (PFMPE_E_ARG), the
// capacities (PFMPE_E_CAP), every image's size, every entry's image index, every entry's parameters as roi_check
// (prm, width, height) judges them (PFMPE_E_ARG, "roi <r>: ...").  Contexts are not looked at.
template <typename RoiCheck>
int check(const pfmpe_detect_image* images, int I, const int32_t* image_of, const pfmpe_detect_params* params, int R,
          RoiCheck&& roi_check, std::string* why) {
  auto bad = [&](int code, const std::string& text) {
    if (why) *why = text;
    return code;
  };
  if (!images || !image_of || !params) return bad(PFMPE_E_ARG, "a null pointer");
  if (I < 1 || R < 1) return bad(PFMPE_E_ARG, "I < 1 or R < 1");
  if (R > PFMPE_DETECT_MAX_ROIS) return bad(PFMPE_E_CAP, "R exceeds PFMPE_DETECT_MAX_ROIS");
  if (I > PFMPE_DETECT_MAX_IMAGES) return bad(PFMPE_E_CAP, "I exceeds PFMPE_DETECT_MAX_IMAGES");
  for (int i = 0; i < I; ++i)
    if (images[i].width < 1 || images[i].height < 1 || images[i].pitch < images[i].width)
      return bad(PFMPE_E_ARG, "image " + std::to_string(i) + ": bad size or pitch");
  for (int r = 0; r < R; ++r) {
    if (image_of[r] < 0 || image_of[r] >= I) return bad(PFMPE_E_ARG, "roi " + std::to_string(r) + ": image index out of range");
    const pfmpe_detect_image& im = images[image_of[r]];
    if (const char* w = roi_check(params + r, im.width, im.height))
      return bad(PFMPE_E_ARG, "roi " + std::to_string(r) + ": " + w);
  }
  return PFMPE_OK;
}

// The plan of a checked batch.  PFMPE_E_CAP when the upload would exceed kMaxUploadBytes (outputs then undefined:
// callers plan into their own storage first).
inline int build(const pfmpe_detect_image* images, const int32_t* image_of, const pfmpe_detect_params* params, int R,
                 pfmpe_detect_crop* crops, int64_t* upload_bytes) {
  Rect rc[PFMPE_DETECT_MAX_ROIS];
  int owner[PFMPE_DETECT_MAX_ROIS];
  for (int r = 0; r < R; ++r) rc[r] = rect_of(params + r, images[image_of[r]].width, images[image_of[r]].height);
  int64_t end = 0;
  for (int r = 0; r < R; ++r) {
    const pfmpe_detect_image& im = images[image_of[r]];
    if (!im.image) {
      owner[r] = -1;
      crops[r] = pfmpe_detect_crop{-1, im.pitch, -1};
      continue;
    }
    int o = r;
    int64_t best = (int64_t)rc[r].w * rc[r].h;
    for (int q = 0; q < R; ++q) {
      if (image_of[q] != image_of[r] || !contains(rc[q], rc[r])) continue;
      const int64_t area = (int64_t)rc[q].w * rc[q].h;
      if (area > best || (area == best && q < o)) {
        o = q;
        best = area;
      }
    }
    owner[r] = o;
    if (o != r) continue;
    const int32_t pitch = (int32_t)(((int64_t)rc[r].w + 15) & ~(int64_t)15);
    crops[r] = pfmpe_detect_crop{end, pitch, -1};
    end = al256(end + (int64_t)rc[r].h * pitch);
    if (end > kMaxUploadBytes) return PFMPE_E_CAP;
  }
  for (int r = 0; r < R; ++r) {  // an owner owns itself, so every owner's crop is final here
    const int q = owner[r];
    if (q < 0 || q == r) continue;
    crops[r].pitch = crops[q].pitch;
    crops[r].shared_with = q;
    crops[r].offset = crops[q].offset + (int64_t)(rc[r].y - rc[q].y) * crops[q].pitch + (rc[r].x - rc[q].x);
  }
  *upload_bytes = end;
  return PFMPE_OK;
}

// The own crops of a checked batch's plan into buffer[0 .. upload_bytes): the rows out of the caller's images, every
// other byte (row tails, alignment gaps) zero.
inline void pack(const pfmpe_detect_image* images, const int32_t* image_of, const pfmpe_detect_params* params, int R,
                 const pfmpe_detect_crop* crops, uint8_t* buffer, int64_t upload_bytes) {
  int64_t at = 0;  // everything below is written
  for (int r = 0; r < R; ++r) {
    const pfmpe_detect_image& im = images[image_of[r]];
    if (!im.image || crops[r].shared_with >= 0) continue;
    const Rect rc = rect_of(params + r, im.width, im.height);
    const int64_t off = crops[r].offset, pitch = crops[r].pitch;
    std::memset(buffer + at, 0, (size_t)(off - at));
    const uint8_t* src = im.image + (int64_t)rc.y * im.pitch + rc.x;
    for (int y = 0; y < rc.h; ++y) {
      uint8_t* dst = buffer + off + y * pitch;
      std::memcpy(dst, src + (int64_t)y * im.pitch, (size_t)rc.w);
      std::memset(dst + rc.w, 0, (size_t)(pitch - rc.w));
    }
    at = off + rc.h * pitch;
  }
  std::memset(buffer + at, 0, (size_t)(upload_bytes - at));
}

}  // namespace pfmpe_plan
