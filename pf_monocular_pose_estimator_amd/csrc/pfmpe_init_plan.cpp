// pfmpe_init_plan.cpp — the host-only entry point of the batch initialisation's work mapping (pfmpe_init_plan.hpp):
// pfmpe_host_init_plan.  No GPU, no context.
#include "pfmpe_init_plan.hpp"

extern "C" {

int pfmpe_host_init_plan(const int32_t* M, const int32_t* B, int S, int num_cu, pfmpe_init_plan* plan,
                         int32_t* blocks_per_bucket) {
  if (!M || !B || !plan || !blocks_per_bucket || S < 1 || S > PFMPE_INIT_MAX_STREAMS) return PFMPE_E_ARG;
  for (int s = 0; s < S; ++s) {
    if (M[s] < 3 || M[s] > PFMPE_MAX_MARKERS || B[s] < 0) return PFMPE_E_ARG;
    if (B[s] > PFMPE_MAX_BLOBS) return PFMPE_E_CAP;
  }
  pfmpe_plan::init_plan(M, B, S, num_cu, plan, blocks_per_bucket);
  return PFMPE_OK;
}

}  // extern "C"
