// pfmpe_detect_plan.cpp — the host-only entry points of the streams detector's upload plan (pfmpe_detect_plan.hpp):
// pfmpe_host_detect_plan and pfmpe_host_detect_pack.  No GPU, no context.
#include "pfmpe_detect_plan.hpp"

extern "C" {

int pfmpe_host_detect_plan(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                           const pfmpe_detect_params* params, int R, pfmpe_detect_crop* crops, int64_t* upload_bytes) {
  if (!crops || !upload_bytes) return PFMPE_E_ARG;
  if (const int rc = pfmpe_plan::check(images, I, image_of, params, R, pfmpe_plan::roi_geometry, nullptr)) return rc;
  pfmpe_detect_crop plan[PFMPE_DETECT_MAX_ROIS];
  int64_t bytes = 0;
  if (const int rc = pfmpe_plan::build(images, image_of, params, R, plan, &bytes)) return rc;
  std::memcpy(crops, plan, (size_t)R * sizeof(*crops));
  *upload_bytes = bytes;
  return PFMPE_OK;
}

// The crops must be the plan of the same batch: they say where this function writes, so they are not taken on trust.
int pfmpe_host_detect_pack(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                           const pfmpe_detect_params* params, int R, const pfmpe_detect_crop* crops, uint8_t* buffer,
                           int64_t buffer_bytes) {
  if (!crops || buffer_bytes < 0) return PFMPE_E_ARG;
  if (const int rc = pfmpe_plan::check(images, I, image_of, params, R, pfmpe_plan::roi_geometry, nullptr)) return rc;
  pfmpe_detect_crop plan[PFMPE_DETECT_MAX_ROIS];
  int64_t bytes = 0;
  if (const int rc = pfmpe_plan::build(images, image_of, params, R, plan, &bytes)) return rc;
  for (int r = 0; r < R; ++r)
    if (crops[r].offset != plan[r].offset || crops[r].pitch != plan[r].pitch || crops[r].shared_with != plan[r].shared_with)
      return PFMPE_E_ARG;
  if (buffer_bytes < bytes) return PFMPE_E_CAP;
  if (bytes == 0) return PFMPE_OK;
  if (!buffer) return PFMPE_E_ARG;
  pfmpe_plan::pack(images, image_of, params, R, plan, buffer, bytes);
  return PFMPE_OK;
}

}  // extern "C"
