// pfmpe_refine_plan.cpp — the host-only entry point of the batch refinement's upload layout (pfmpe_refine_plan.hpp):
// pfmpe_host_refine_plan.  No GPU, no context.
#include "pfmpe_refine_plan.hpp"

extern "C" {

int pfmpe_host_refine_plan(const int32_t* K, const int32_t* B, int S, pfmpe_refine_plan* plan,
                           pfmpe_refine_plan_total* total) {
  if (!K || !B || !plan || !total || S < 1) return PFMPE_E_ARG;
  if (S > PFMPE_REFINE_MAX_STREAMS) return PFMPE_E_CAP;
  int64_t H = 0;
  for (int s = 0; s < S; ++s) {
    if (K[s] < 0 || B[s] < 0) return PFMPE_E_ARG;
    if (B[s] > PFMPE_MAX_BLOBS) return PFMPE_E_CAP;
    H += K[s];
  }
  if (H > PFMPE_REFINE_MULTI_MAX_HYPOTHESES) return PFMPE_E_CAP;
  pfmpe_plan::refine_plan(K, B, S, plan, total);
  return PFMPE_OK;
}

}  // extern "C"
