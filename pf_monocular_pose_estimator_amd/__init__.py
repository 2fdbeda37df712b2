"""pf_monocular_pose_estimator_amd — MI355X-native particle-filter pose engine.

The hot path of ObiRobotics/pf_monocular_pose_estimator (the PF step of PoseEstimator::estimateBodyPose,
pf_mpe_lib/src/pose_estimator.cpp:475-733) as hand-written HIP for gfx950 behind the C-ABI in
include/pfmpe.h.  This package holds the in-tree built library (libpfmpe.so), its ctypes binding
(`_capi`), and the synthetic stream generator used by tests and bench.py.
"""
from ._capi import (  # noqa: F401
    Engine, FrameIn, FrameOut, Params, PFError, default_params, load, host_philox, host_ref_uniform,
    STATE_F32, STATE_F64, STATE_F16, RNG_REFERENCE, RNG_PHILOX, FLAG_ACCEPTED, FLAG_REINIT,
    OPT_RECORD_COUNTS, OPT_PRUNE, OPT_TIMING, OPT_FUSED, OPT_KEEP_PROPAGATED, K_FRAME, K_ROI, K_FINAL, MAX_MARKERS, MAX_BLOBS, LIB_PATH,
    OPT_WAIT_BOUND_US, OPT_FUSED_REARM, OPT_MULTI_MAX_BLOCKS, OPT_DIAG, DIAG_LAG_LOADS, DIAG_ABANDON, DIAG_NO_STREAM, DIAG_FORCE_STREAM,
    DIAG_SERIAL_TOP, DIAG_NO_PK, DIAG_CORRUPT_DESC, DIAG_NO_DEFER, DIAG_BLOCK_RESAMPLE, DIAG_MIN_SIDE, DIAG_ABANDON_FINISH, OPT_DEFER_RESAMPLE, OK, E_ARG, E_HIP, E_CAP, E_STATE,
    SHAPE_TWO_LAUNCH, SHAPE_FRAME, SHAPE_FRAME2, INFO_FUSED, INFO_FUSED_FALLBACKS, INFO_LAST_SHAPE,
    INFO_GUARD_SKIPS, INFO_N, INFO_LAST_WEIGH_PASS, INFO_LAST_GRID, INFO_LAST_RESAMPLE, RESAMPLE_BLOCKS, RESAMPLE_OWNERS, WEIGH_BLOCKS, WEIGH_STREAM, WEIGH_PK,
    CLOUD_WEIGHTED, CLOUD_POSTERIOR, CloudOut, host_pose_twist,
    ASSOC_PROPAGATED, ASSOC_POSTERIOR, DIAG_ASSOC_DIRECT, AssocIn, AssocOut, host_assoc_summary,
    REFINE_NO_PAIRS, REFINE_CONVERGED, REFINE_CAP_KEPT, REFINE_CAP_REVERTED, REFINE_ROW_DTYPE, RefineParams, RefineRow,
    RefineOut, default_refine_params, host_optimise_pose,
    DETECT_MAX_ROIS, DetectParams, DetectOut, host_grow_roi,
    ROI_MAX_STREAMS, RoiIn, RoiOut, host_predict_roi,
    DETECT_MAX_IMAGES, DIAG_DET_COPY, DetectImage, DetectCrop, host_detect_plan, host_detect_pack,
    INIT_MAX_STREAMS, INFO_NUM_CU, InitIn, InitPlan, InitParams, InitOut, host_init_plan,
    REFINE_MAX_STREAMS, REFINE_MULTI_MAX_HYPOTHESES, REFINE_DESC_BYTES, RefineIn, RefinePlan, RefinePlanTotal,
    host_refine_plan,
    DIAG_TAIL_MISS, INFO_TAIL_FALLBACKS, host_step_tail,
    CLOUD_MAX_STREAMS, CloudIn, CloudPlan, host_cloud_plan,
    TOP_MAX, TOP_POOL, TOP_BY_WEIGHT, TOP_BY_COUNT, TopParams, TopOut, default_top_params, host_top_suppress,
    MODES_MAX, MODE_NONE, ModesParams, ModeOut, default_modes_params, host_cloud_assign,
    ResampleParams, ResampleOut, host_resample_source, host_resample_rank,
    ASSOC_MAX_STREAMS, ASSOC_MAX_LAUNCHES, AssocMultiIn, AssocPlan, AssocPlanTotal, host_assoc_plan,
    GateParams, GateOut, default_gate_params, host_gate_pairs,
)

__all__ = [
    "Engine", "FrameIn", "FrameOut", "Params", "PFError", "default_params", "load",
    "STATE_F32", "STATE_F64", "RNG_REFERENCE", "RNG_PHILOX",
]
