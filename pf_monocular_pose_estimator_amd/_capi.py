"""ctypes binding of the C-ABI in include/pfmpe.h (libpfmpe.so, built in-tree by __graft_entry__.build()).

This is the same boundary a reference-side maintainer would bind; it loads ONLY the
HIP-built product library and raises if it is missing — there is no CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpfmpe.so")

MAX_MARKERS = 16
MAX_BLOBS = 1024

OK, E_ARG, E_HIP, E_CAP, E_STATE = 0, -1, -2, -3, -4
STATE_F32, STATE_F64, STATE_F16 = 0, 1, 2
RNG_REFERENCE, RNG_PHILOX = 0, 1
FLAG_ACCEPTED, FLAG_REINIT = 1, 4
OPT_RECORD_COUNTS, OPT_PRUNE, OPT_TIMING, OPT_FUSED, OPT_KEEP_PROPAGATED = 1, 2, 3, 4, 5
OPT_WAIT_BOUND_US, OPT_FUSED_REARM, OPT_MULTI_MAX_BLOCKS = 6, 7, 8
OPT_DIAG = 99  # undocumented diagnostic switches (csrc/pf_types.hpp kDiag*)
DIAG_LAG_LOADS, DIAG_ABANDON, DIAG_NO_STREAM, DIAG_FORCE_STREAM, DIAG_SERIAL_TOP = 64, 128, 512, 1024, 2048
DIAG_NO_PK, DIAG_CORRUPT_DESC, DIAG_NO_DEFER, DIAG_BLOCK_RESAMPLE, DIAG_MIN_SIDE = 4096, 8192, 16384, 32768, 65536
DIAG_ABANDON_FINISH = 131072
DIAG_DET_COPY = 524288  # find_leds_streams: the crops go up by one async copy command instead of the pull kernel (A/B)
DIAG_TAIL_MISS = 1 << 20  # step_refine(_multi): the tail reports "record not ready" (the recovery path)
DIAG_ASSOC_DIRECT = 262144  # assoc_stats: every vote straight into the device table (the path of tables too large for LDS)
OPT_DEFER_RESAMPLE = 9
SHAPE_TWO_LAUNCH, SHAPE_FRAME, SHAPE_FRAME2 = 0, 1, 2
INFO_FUSED, INFO_FUSED_FALLBACKS, INFO_LAST_SHAPE, INFO_GUARD_SKIPS, INFO_N, INFO_LAST_WEIGH_PASS = 1, 2, 3, 4, 5, 6
INFO_LAST_GRID, INFO_LAST_RESAMPLE, INFO_NUM_CU, INFO_TAIL_FALLBACKS = 7, 8, 9, 10
WEIGH_BLOCKS, WEIGH_STREAM, WEIGH_PK = 0, 1, 2
RESAMPLE_BLOCKS, RESAMPLE_OWNERS = 0, 1
CLOUD_WEIGHTED, CLOUD_POSTERIOR = 0, 1
ASSOC_PROPAGATED, ASSOC_POSTERIOR = 0, 1
REFINE_NO_PAIRS, REFINE_CONVERGED, REFINE_CAP_KEPT, REFINE_CAP_REVERTED = 0, 1, 2, 3
K_PROPAGATE, K_RESAMPLE, K_AUX, K_FRAME, K_ROI, K_FINAL, K_P3P_HIST, K_P3P_CHECK, K_DETECT, K_COUNT = range(10)

# every symbol include/pfmpe.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    "pfmpe_create", "pfmpe_destroy", "pfmpe_last_error", "pfmpe_abi_version",
    "pfmpe_set_model", "pfmpe_set_params", "pfmpe_default_params", "pfmpe_set_prior",
    "pfmpe_step", "pfmpe_step_batch", "pfmpe_step_multi", "pfmpe_step_multi_batch", "pfmpe_get_particles", "pfmpe_get_weights", "pfmpe_get_counts",
    "pfmpe_set_option", "pfmpe_stage_blob_bank", "pfmpe_get_kernel_stats",
    "pfmpe_reset_kernel_stats", "pfmpe_kernel_name", "pfmpe_host_ref_uniform", "pfmpe_host_philox",
    "pfmpe_predict_roi", "pfmpe_default_init_params", "pfmpe_p3p_histogram", "pfmpe_initialise",
    "pfmpe_parse_marker_yaml", "pfmpe_default_launch_config", "pfmpe_parse_launch", "pfmpe_parse_camera_info",
    "pfmpe_write_blob_stream", "pfmpe_read_blob_stream", "pfmpe_stage_blob_stream",
    "pfmpe_default_detect_params", "pfmpe_stage_image", "pfmpe_find_leds", "pfmpe_get_info",
    "pfmpe_cloud_stats", "pfmpe_host_pose_twist",
    "pfmpe_assoc_stats", "pfmpe_get_pairs", "pfmpe_host_assoc_summary",
    "pfmpe_default_refine_params", "pfmpe_refine_poses", "pfmpe_refine_cloud", "pfmpe_host_optimise_pose",
    "pfmpe_find_leds_multi", "pfmpe_host_grow_roi",
    "pfmpe_predict_roi_multi", "pfmpe_host_predict_roi",
    "pfmpe_find_leds_streams", "pfmpe_host_detect_plan", "pfmpe_host_detect_pack",
    "pfmpe_initialise_multi", "pfmpe_host_init_plan",
    "pfmpe_refine_multi", "pfmpe_host_refine_plan",
    "pfmpe_step_refine", "pfmpe_step_refine_multi", "pfmpe_host_step_tail",
    "pfmpe_cloud_stats_multi", "pfmpe_host_cloud_plan",
    "pfmpe_default_top_params", "pfmpe_top_particles", "pfmpe_host_top_suppress",
    "pfmpe_default_modes_params", "pfmpe_cloud_modes", "pfmpe_host_cloud_assign",
    "pfmpe_resample_prior", "pfmpe_host_resample_source", "pfmpe_host_resample_rank",
    "pfmpe_assoc_stats_multi", "pfmpe_host_assoc_plan", "pfmpe_default_gate_params", "pfmpe_host_gate_pairs",
)
MODES_MAX = 16
MODE_NONE = 255
TOP_MAX = 1024
TOP_POOL = 1024
TOP_BY_WEIGHT, TOP_BY_COUNT = 0, 1
DETECT_MAX_ROIS = 64
DETECT_MAX_IMAGES = 64
ROI_MAX_STREAMS = 64
INIT_MAX_STREAMS = 64
REFINE_MAX_STREAMS = 64
CLOUD_MAX_STREAMS = 64
ASSOC_MAX_STREAMS = 64
ASSOC_MAX_LAUNCHES = 16
REFINE_MULTI_MAX_HYPOTHESES = 65536
REFINE_DESC_BYTES = 48


class Params(C.Structure):
    _fields_ = [
        ("tol", C.c_double), ("tol_pf", C.c_double),
        ("ang_min", C.c_double), ("ang_max", C.c_double),
        ("trans_min", C.c_double), ("trans_max", C.c_double),
        ("growth", C.c_double),
        ("max_iter", C.c_int32), ("exit_cap", C.c_int32), ("accept_cap", C.c_int32),
        ("rng_mode", C.c_int32),
    ]


class FrameIn(C.Structure):
    _fields_ = [
        ("current_pose", C.c_double * 12), ("predicted_pose", C.c_double * 12),
        ("prediction", C.c_double * 12), ("cam_move_inv", C.c_double * 12),
        ("blobs", C.POINTER(C.c_double)), ("B", C.c_int32), ("bank_frame", C.c_int32),
        ("it_since_init", C.c_int32), ("force_iters", C.c_int32),
        ("dt", C.c_double), ("seed", C.c_uint64), ("frame_idx", C.c_uint64),
    ]


class RoiIn(C.Structure):
    _fields_ = [
        ("cam_move_inv", C.c_double * 12), ("prediction", C.c_double * 12), ("predicted_pose", C.c_double * 12),
        ("D", C.c_double * 5), ("image_w", C.c_int32), ("image_h", C.c_int32), ("border", C.c_int32),
        ("pad", C.c_int32),
    ]


class RoiOut(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("bbox", C.c_double * 4)]


class InitParams(C.Structure):
    _fields_ = [("certainty_threshold", C.c_double), ("valid_corr_threshold", C.c_double),
                ("n_particles", C.c_int32), ("max_candidates", C.c_int32)]


class InitOut(C.Structure):
    _fields_ = [("found", C.c_int32), ("flag_fail", C.c_int32), ("n_estimates", C.c_int32),
                ("n_candidates", C.c_int32), ("first_match", C.c_int32), ("n_corr", C.c_int32),
                ("corr", C.c_uint32 * (2 * MAX_MARKERS)), ("predicted_pose", C.c_double * 12),
                ("hist_total", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"found": self.found, "flag_fail": self.flag_fail, "n_estimates": self.n_estimates,
                "n_candidates": self.n_candidates, "first_match": self.first_match,
                "pairs": np.array(self.corr[: 2 * self.n_corr], dtype=np.uint32).reshape(-1, 2),
                "predicted_pose": np.array(self.predicted_pose), "hist_total": self.hist_total}


class InitIn(C.Structure):
    _fields_ = [("blobs", C.POINTER(C.c_double)), ("B", C.c_int32), ("pad", C.c_int32)]


class InitPlan(C.Structure):
    _fields_ = [("items", C.c_int64), ("first_block", C.c_int32), ("blocks", C.c_int32), ("bucket", C.c_int32),
                ("lds_hist", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class DetectParams(C.Structure):
    _fields_ = [("threshold_value", C.c_int32), ("active_markers", C.c_int32), ("gaussian_sigma", C.c_double),
                ("min_blob_area", C.c_double), ("max_blob_area", C.c_double),
                ("max_width_height_distortion", C.c_double), ("max_circular_distortion", C.c_double),
                ("D", C.c_double * 5), ("roi_x", C.c_int32), ("roi_y", C.c_int32), ("roi_w", C.c_int32),
                ("roi_h", C.c_int32)]


class DetectOut(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_components", C.c_int32), ("overflow", C.c_int32), ("pad", C.c_int32)]


class DetectImage(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("image", C.POINTER(C.c_uint8)), ("width", C.c_int32), ("height", C.c_int32),
                ("pitch", C.c_int32), ("pad", C.c_int32)]


class DetectCrop(C.Structure):
    _fields_ = [("offset", C.c_int64), ("pitch", C.c_int32), ("shared_with", C.c_int32)]


class LaunchConfig(C.Structure):
    _fields_ = [("pf", Params), ("init", InitParams), ("num_objects", C.c_int32),
                ("markers_per_object", C.c_int32 * 4), ("use_particle_filter", C.c_int32),
                ("downgrade", C.c_uint8 * MAX_MARKERS)]


class FrameOut(C.Structure):
    _fields_ = [
        ("iters", C.c_int32), ("kept_iter", C.c_int32), ("most_likely_idx", C.c_int32),
        ("accepted", C.c_int32), ("resampled", C.c_int32), ("winner_idx", C.c_int32),
        ("n_corr", C.c_int32), ("flag_fail", C.c_int32),
        ("highest_prob", C.c_double), ("prob_sum", C.c_double),
        ("winner_pose", C.c_double * 12), ("most_likely_pose", C.c_double * 12),
        ("corr", C.c_uint32 * (2 * MAX_MARKERS)),
    ]

    def pairs(self) -> np.ndarray:
        return np.array(self.corr[: 2 * self.n_corr], dtype=np.uint32).reshape(-1, 2)

    def as_dict(self) -> dict:
        return {
            "iters": self.iters, "kept_iter": self.kept_iter, "most_likely_idx": self.most_likely_idx,
            "accepted": self.accepted, "resampled": self.resampled, "winner_idx": self.winner_idx,
            "n_corr": self.n_corr, "flag_fail": self.flag_fail, "highest_prob": self.highest_prob,
            "prob_sum": self.prob_sum, "winner_pose": np.array(self.winner_pose),
            "most_likely_pose": np.array(self.most_likely_pose), "pairs": self.pairs(),
        }


class CloudOut(C.Structure):
    _fields_ = [("n", C.c_int64), ("degenerate", C.c_int32), ("pad", C.c_int32),
                ("wsum", C.c_double), ("ess", C.c_double), ("mean_twist", C.c_double * 6),
                ("cov", C.c_double * 36), ("mean_pose", C.c_double * 12),
                ("max_trans", C.c_double), ("max_rot", C.c_double)]

    def as_dict(self) -> dict:
        return {"n": self.n, "degenerate": self.degenerate, "wsum": self.wsum, "ess": self.ess,
                "mean_twist": np.array(self.mean_twist), "cov": np.array(self.cov).reshape(6, 6),
                "mean_pose": np.array(self.mean_pose), "max_trans": self.max_trans, "max_rot": self.max_rot}


class CloudIn(C.Structure):
    _fields_ = [("ref_pose", C.c_double * 12), ("which", C.c_int32), ("pad", C.c_int32)]


class CloudPlan(C.Structure):
    _fields_ = [("first_block", C.c_int32), ("blocks", C.c_int32)]

    def as_dict(self) -> dict:
        return {"first_block": self.first_block, "blocks": self.blocks}


class ModesParams(C.Structure):
    _fields_ = [("trans_scale", C.c_double), ("rot_scale", C.c_double), ("max_dist", C.c_double)]


class ModeOut(C.Structure):
    _fields_ = [("stats", CloudOut), ("share", C.c_double)]

    def as_dict(self) -> dict:
        d = self.stats.as_dict()
        d["share"] = self.share
        return d


# the sizes include/pfmpe.h states (pfmpe_engine.hip asserts them on its side)
assert C.sizeof(ModesParams) == 24 and C.sizeof(CloudOut) == 480 and C.sizeof(ModeOut) == 488


class ResampleParams(C.Structure):
    _fields_ = [("n_new", C.c_int32), ("K", C.c_int32), ("seeds", C.POINTER(C.c_double)), ("mode", C.c_int32),
                ("pad", C.c_int32), ("modes", ModesParams)]


class ResampleOut(C.Structure):
    _fields_ = [("n_src", C.c_int64), ("n_members", C.c_int64), ("n_new", C.c_int64)]

    def as_dict(self) -> dict:
        return {"n_src": self.n_src, "n_members": self.n_members, "n_new": self.n_new}


assert C.sizeof(ResampleParams) == 48 and C.sizeof(ResampleOut) == 24


class AssocIn(C.Structure):
    _fields_ = [("blobs", C.POINTER(C.c_double)), ("B", C.c_int32), ("bank_frame", C.c_int32)]


class AssocOut(C.Structure):
    _fields_ = [("n", C.c_int64), ("M", C.c_int32), ("B", C.c_int32), ("n_any", C.c_int64),
                ("matched", C.c_uint32 * MAX_MARKERS), ("mode_blob", C.c_uint32 * MAX_MARKERS),
                ("mode_votes", C.c_uint32 * MAX_MARKERS), ("second_votes", C.c_uint32 * MAX_MARKERS),
                ("npairs_hist", C.c_uint32 * (MAX_MARKERS + 1)), ("pad", C.c_uint32)]

    def as_dict(self) -> dict:
        """The arrays trimmed to the M LEDs (npairs_hist to M + 1 counts)."""
        M = self.M
        d = {"n": self.n, "M": M, "B": self.B, "n_any": self.n_any}
        for k in ("matched", "mode_blob", "mode_votes", "second_votes"):
            d[k] = np.array(getattr(self, k)[:M], dtype=np.uint32)
        d["npairs_hist"] = np.array(self.npairs_hist[: M + 1], dtype=np.uint32)
        return d


class AssocMultiIn(C.Structure):
    _fields_ = [("blobs", AssocIn), ("which", C.c_int32), ("pad", C.c_int32)]


class AssocPlan(C.Structure):
    _fields_ = [("bins_offset", C.c_int64), ("first_block", C.c_int32), ("blocks", C.c_int32),
                ("launch", C.c_int32), ("lds_votes", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class AssocPlanTotal(C.Structure):
    _fields_ = [("bins_words", C.c_int64), ("launches", C.c_int32), ("pad", C.c_int32),
                ("launch_blocks", C.c_int32 * ASSOC_MAX_LAUNCHES)]

    def as_dict(self) -> dict:
        return {"bins_words": self.bins_words, "launches": self.launches,
                "launch_blocks": list(self.launch_blocks[: self.launches])}


class GateParams(C.Structure):
    _fields_ = [("min_share", C.c_double), ("lead", C.c_double), ("min_pairs", C.c_int32), ("pad", C.c_int32)]


class GateOut(C.Structure):
    _fields_ = [("n_in", C.c_int32), ("n_gated", C.c_int32), ("fallback", C.c_int32), ("pad", C.c_int32),
                ("reason", C.c_uint8 * MAX_MARKERS)]


# the sizes include/pfmpe.h states (pfmpe_engine.hip asserts them on its side)
assert (C.sizeof(AssocMultiIn), C.sizeof(AssocPlan), C.sizeof(AssocPlanTotal), C.sizeof(GateParams),
        C.sizeof(GateOut)) == (24, 24, 80, 24, 32)


class TopParams(C.Structure):
    _fields_ = [("key", C.c_int32), ("K", C.c_int32), ("min_trans", C.c_double), ("min_rot", C.c_double)]


class TopOut(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_positive", C.c_int64), ("n_out", C.c_int32), ("n_examined", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class RefineParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("revert_on_divergence", C.c_int32), ("converged", C.c_double)]


class RefineRow(C.Structure):
    _fields_ = [("pose", C.c_double * 12), ("rms_before", C.c_double), ("rms_after", C.c_double),
                ("iters", C.c_int32), ("n_pairs", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


# pfmpe_refine_row as a numpy record (128 bytes)
REFINE_ROW_DTYPE = np.dtype([("pose", np.float64, 12), ("rms_before", np.float64), ("rms_after", np.float64),
                             ("iters", np.int32), ("n_pairs", np.int32), ("status", np.int32), ("pad", np.int32)])


class RefineOut(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_with_pairs", C.c_int64), ("n_converged", C.c_int64), ("n_cap_kept", C.c_int64),
                ("n_cap_reverted", C.c_int64), ("iters_total", C.c_int64), ("iters_max", C.c_int32), ("pad", C.c_int32),
                ("best", C.c_int64), ("best_row", RefineRow), ("best_cov", C.c_double * 36)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in ("n", "n_with_pairs", "n_converged", "n_cap_kept", "n_cap_reverted",
                                           "iters_total", "iters_max", "best")}
        d["best_row"] = np.frombuffer(bytes(self.best_row), dtype=REFINE_ROW_DTYPE)[0].copy()
        d["best_cov"] = np.array(self.best_cov).reshape(6, 6)
        return d


class RefineIn(C.Structure):
    _fields_ = [("blobs", AssocIn), ("poses", C.POINTER(C.c_double)), ("corr", C.POINTER(C.c_uint32)),
                ("K", C.c_int32), ("pad", C.c_int32)]


class RefinePlan(C.Structure):
    _fields_ = [("first", C.c_int64), ("model_offset", C.c_int64), ("blobs_offset", C.c_int64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class RefinePlanTotal(C.Structure):
    _fields_ = [("hypotheses", C.c_int64), ("desc_offset", C.c_int64), ("stream_of_offset", C.c_int64),
                ("poses_offset", C.c_int64), ("corr_offset", C.c_int64), ("upload_bytes", C.c_int64),
                ("download_bytes", C.c_int64)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load() -> C.CDLL:
    """Load libpfmpe.so (raises if it has not been built: the product has no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()')"
        )
    lib = C.CDLL(os.environ.get("PFMPE_LIB_OVERRIDE") or LIB_PATH)  # override: A/B builds of the same ABI
    P, I, D, U64, I64 = C.c_void_p, C.c_int, C.c_double, C.c_uint64, C.c_int64
    dp = C.POINTER(C.c_double)
    sig = {
        "pfmpe_create": (I, [C.POINTER(P), I, I, I, I, I]),
        "pfmpe_destroy": (None, [P]),
        "pfmpe_last_error": (C.c_char_p, [P]),
        "pfmpe_abi_version": (I, []),
        "pfmpe_set_model": (I, [P, dp, I, dp, C.POINTER(C.c_uint8)]),
        "pfmpe_set_params": (I, [P, C.POINTER(Params)]),
        "pfmpe_default_params": (None, [C.POINTER(Params)]),
        "pfmpe_set_prior": (I, [P, dp, I]),
        "pfmpe_step": (I, [P, C.POINTER(FrameIn), C.POINTER(FrameOut)]),
        "pfmpe_step_batch": (I, [P, C.POINTER(FrameIn), I, C.POINTER(FrameOut), C.POINTER(I)]),
        "pfmpe_step_multi": (I, [C.POINTER(P), I, C.POINTER(FrameIn), C.POINTER(FrameOut)]),
        "pfmpe_step_multi_batch": (I, [C.POINTER(P), I, C.POINTER(FrameIn), I, C.POINTER(FrameOut), C.POINTER(I)]),
        "pfmpe_get_particles": (I, [P, I, dp]),
        "pfmpe_get_weights": (I, [P, dp]),
        "pfmpe_get_counts": (I, [P, C.POINTER(C.c_uint32)]),
        "pfmpe_set_option": (I, [P, I, I64]),
        "pfmpe_get_info": (I, [P, I, C.POINTER(I64)]),
        "pfmpe_stage_blob_bank": (I, [P, dp, C.POINTER(C.c_int32), I]),
        "pfmpe_get_kernel_stats": (I, [P, I, C.POINTER(I64), dp]),
        "pfmpe_reset_kernel_stats": (I, [P]),
        "pfmpe_kernel_name": (C.c_char_p, [I]),
        "pfmpe_host_ref_uniform": (D, [C.c_uint32, U64, D, D]),
        "pfmpe_host_philox": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "pfmpe_host_pose_twist": (None, [dp, dp, dp]),
        "pfmpe_cloud_stats": (I, [P, I, dp, C.POINTER(CloudOut)]),
        "pfmpe_cloud_stats_multi": (I, [C.POINTER(P), I, C.POINTER(CloudIn), C.POINTER(CloudOut)]),
        "pfmpe_host_cloud_plan": (I, [C.POINTER(C.c_int32), I, C.POINTER(CloudPlan), C.POINTER(C.c_int32)]),
        "pfmpe_assoc_stats": (I, [P, I, C.POINTER(AssocIn), C.POINTER(AssocOut), C.POINTER(C.c_uint32)]),
        "pfmpe_get_pairs": (I, [P, I, C.POINTER(AssocIn), C.c_int64, C.c_int32, C.POINTER(C.c_uint32),
                                C.POINTER(C.c_int32)]),
        "pfmpe_host_assoc_summary": (I, [C.POINTER(C.c_uint32), I, I, C.POINTER(AssocOut)]),
        "pfmpe_assoc_stats_multi": (I, [C.POINTER(P), I, C.POINTER(AssocMultiIn), C.POINTER(AssocOut),
                                        C.POINTER(C.POINTER(C.c_uint32))]),
        "pfmpe_host_assoc_plan": (I, [C.POINTER(C.c_int32)] * 6 + [I, I, C.POINTER(AssocPlan), C.POINTER(AssocPlanTotal)]),
        "pfmpe_default_gate_params": (None, [C.POINTER(GateParams)]),
        "pfmpe_host_gate_pairs": (I, [C.POINTER(C.c_uint32), I, I, C.POINTER(C.c_uint32), I, C.POINTER(GateParams),
                                      C.POINTER(C.c_uint32), C.POINTER(GateOut)]),
        "pfmpe_default_top_params": (None, [C.POINTER(TopParams)]),
        "pfmpe_top_particles": (I, [P, C.POINTER(TopParams), C.POINTER(AssocIn), C.POINTER(TopOut), C.POINTER(C.c_int32),
                                    dp, dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
        "pfmpe_host_top_suppress": (I, [dp, C.c_int32, C.c_int32, D, D, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
        "pfmpe_default_modes_params": (None, [C.POINTER(ModesParams)]),
        "pfmpe_cloud_modes": (I, [P, I, dp, I, C.POINTER(ModesParams), C.POINTER(ModeOut), C.POINTER(C.c_uint8)]),
        "pfmpe_host_cloud_assign": (I, [dp, I64, dp, I, C.POINTER(ModesParams), C.POINTER(C.c_uint8),
                                        C.POINTER(I64)]),
        "pfmpe_resample_prior": (I, [P, P, C.POINTER(ResampleParams), C.POINTER(ResampleOut)]),
        "pfmpe_host_resample_source": (I, [C.POINTER(C.c_uint8), I64, C.c_int32, I64, C.POINTER(C.c_int32),
                                           C.POINTER(I64)]),
        "pfmpe_host_resample_rank": (I, [I64, I64, I64, C.POINTER(I64)]),
        "pfmpe_default_refine_params": (None, [C.POINTER(RefineParams)]),
        "pfmpe_refine_poses": (I, [P, C.POINTER(AssocIn), C.POINTER(RefineParams), dp, C.POINTER(C.c_uint32), C.c_int32,
                                   C.POINTER(RefineOut), P, dp]),
        "pfmpe_refine_cloud": (I, [P, I, C.POINTER(AssocIn), C.POINTER(RefineParams), C.c_int64, C.c_int32,
                                   C.POINTER(RefineOut), P, dp]),
        "pfmpe_host_optimise_pose": (I, [dp, I, dp, dp, I, C.POINTER(C.c_uint32), I, C.POINTER(RefineParams), dp,
                                         C.POINTER(RefineRow), dp]),
        "pfmpe_refine_multi": (I, [C.POINTER(P), I, C.POINTER(RefineIn), C.POINTER(RefineParams), C.POINTER(RefineOut),
                                   C.POINTER(P), C.POINTER(dp)]),
        "pfmpe_host_refine_plan": (I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), I, C.POINTER(RefinePlan),
                                       C.POINTER(RefinePlanTotal)]),
        "pfmpe_step_refine": (I, [P, C.POINTER(FrameIn), C.POINTER(RefineParams), C.POINTER(FrameOut),
                                  C.POINTER(RefineOut), C.POINTER(RefineRow), dp]),
        "pfmpe_step_refine_multi": (I, [C.POINTER(P), I, C.POINTER(FrameIn), C.POINTER(RefineParams), C.POINTER(FrameOut),
                                        C.POINTER(RefineOut), C.POINTER(RefineRow), dp]),
        "pfmpe_host_step_tail": (I, [dp, I, dp, dp, I, C.POINTER(FrameOut), C.POINTER(RefineParams), C.POINTER(RefineOut),
                                     C.POINTER(RefineRow), dp]),
        "pfmpe_predict_roi": (I, [P, C.POINTER(RoiIn), C.POINTER(RoiOut)]),
        "pfmpe_predict_roi_multi": (I, [C.POINTER(P), I, C.POINTER(RoiIn), C.POINTER(RoiOut)]),
        "pfmpe_host_predict_roi": (I, [dp, I, dp, dp, I64, C.POINTER(RoiIn), C.POINTER(RoiOut)]),
        "pfmpe_default_init_params": (None, [C.POINTER(InitParams)]),
        "pfmpe_p3p_histogram": (I, [P, dp, I, C.POINTER(C.c_uint32)]),
        "pfmpe_initialise": (I, [P, dp, I, C.POINTER(InitParams), C.POINTER(InitOut), C.POINTER(C.c_uint32)]),
        "pfmpe_initialise_multi": (I, [C.POINTER(P), I, C.POINTER(InitIn), C.POINTER(InitParams), C.POINTER(InitOut),
                                       C.POINTER(C.POINTER(C.c_uint32))]),
        "pfmpe_host_init_plan": (I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), I, I, C.POINTER(InitPlan),
                                     C.POINTER(C.c_int32)]),
        "pfmpe_parse_marker_yaml": (I, [C.c_char_p, dp, I]),
        "pfmpe_default_launch_config": (None, [C.POINTER(LaunchConfig)]),
        "pfmpe_parse_launch": (I, [C.c_char_p, C.POINTER(LaunchConfig)]),
        "pfmpe_parse_camera_info": (I, [C.c_char_p, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "pfmpe_write_blob_stream": (I, [C.c_char_p, dp, dp, C.POINTER(C.c_int32), I]),
        "pfmpe_read_blob_stream": (I, [C.c_char_p, dp, dp, C.POINTER(C.c_int32), I, I64, C.POINTER(I),
                                       C.POINTER(I64)]),
        "pfmpe_stage_blob_stream": (I, [P, C.c_char_p, C.POINTER(I)]),
        "pfmpe_default_detect_params": (None, [C.POINTER(DetectParams)]),
        "pfmpe_stage_image": (I, [P, C.POINTER(C.c_uint8), I, I, I]),
        "pfmpe_find_leds": (I, [P, C.POINTER(C.c_uint8), I, I, I, C.POINTER(DetectParams), dp,
                                C.POINTER(C.c_float), I, C.POINTER(DetectOut)]),
        "pfmpe_find_leds_multi": (I, [P, C.POINTER(C.c_uint8), I, I, I, C.POINTER(DetectParams), I, dp,
                                      C.POINTER(C.c_float), I, C.POINTER(DetectOut)]),
        "pfmpe_host_grow_roi": (I, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
        "pfmpe_find_leds_streams": (I, [C.POINTER(DetectImage), I, C.POINTER(C.c_int32), C.POINTER(DetectParams), I, dp,
                                        C.POINTER(C.c_float), I, C.POINTER(DetectOut)]),
        "pfmpe_host_detect_plan": (I, [C.POINTER(DetectImage), I, C.POINTER(C.c_int32), C.POINTER(DetectParams), I,
                                       C.POINTER(DetectCrop), C.POINTER(I64)]),
        "pfmpe_host_detect_pack": (I, [C.POINTER(DetectImage), I, C.POINTER(C.c_int32), C.POINTER(DetectParams), I,
                                       C.POINTER(DetectCrop), C.POINTER(C.c_uint8), I64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def default_params() -> Params:
    p = Params()
    load().pfmpe_default_params(C.byref(p))
    return p


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class PFError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pfmpe error {code}: {msg}")
        self.code = code


class Engine:
    """One PF context (one camera stream / tracked object) on one HIP device."""

    def __init__(self, device: int = 0, max_particles: int = 1000, max_markers: int = MAX_MARKERS,
                 max_blobs: int = MAX_BLOBS, state_dtype: int = STATE_F32):
        self.lib = load()
        self.ctx = C.c_void_p()
        rc = self.lib.pfmpe_create(C.byref(self.ctx), device, max_particles, max_markers, max_blobs, state_dtype)
        if rc != OK:
            raise PFError(rc, "pfmpe_create failed (no HIP device?)")
        self.state_dtype = state_dtype
        self.max_particles = max_particles
        self.N = 0
        self.M = 0
        self._last_out = None  # the last step's FrameOut (cloud_stats' default reference)

    def close(self):
        if self.ctx:
            self.lib.pfmpe_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != OK:
            raise PFError(rc, self.lib.pfmpe_last_error(self.ctx).decode())

    def set_model(self, markers: np.ndarray, K: np.ndarray, downgrade=None):
        m = np.ascontiguousarray(markers, dtype=np.float64).reshape(-1, 3)
        k = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        dg = None
        if downgrade is not None:
            dga = np.ascontiguousarray(downgrade, dtype=np.uint8)
            dg = dga.ctypes.data_as(C.POINTER(C.c_uint8))
        self._chk(self.lib.pfmpe_set_model(self.ctx, _dptr(m), m.shape[0], _dptr(k), dg))
        self.M = m.shape[0]

    def set_params(self, params: Params):
        self._chk(self.lib.pfmpe_set_params(self.ctx, C.byref(params)))

    def set_option(self, opt: int, value: int):
        self._chk(self.lib.pfmpe_set_option(self.ctx, opt, int(value)))

    def info(self, key: int) -> int:
        v = C.c_int64()
        self._chk(self.lib.pfmpe_get_info(self.ctx, key, C.byref(v)))
        return v.value

    def last_error(self) -> str:
        return self.lib.pfmpe_last_error(self.ctx).decode()

    def set_prior(self, poses: np.ndarray):
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
        self._chk(self.lib.pfmpe_set_prior(self.ctx, _dptr(p), p.shape[0]))
        self.N = p.shape[0]
        self._last_out = None

    def stage_blob_bank(self, frames):
        offs = np.zeros(len(frames) + 1, dtype=np.int32)
        for i, f in enumerate(frames):
            offs[i + 1] = offs[i] + len(f)
        allb = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float64).reshape(-1, 2) for f in frames]
                                                   + [np.zeros((0, 2))]), dtype=np.float64)
        self._bank_keep = allb
        self._chk(self.lib.pfmpe_stage_blob_bank(self.ctx, _dptr(allb), offs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 len(frames)))

    @staticmethod
    def make_frame(current_pose, predicted_pose, prediction, blobs=None, B=None, cam_move_inv=None,
                   it_since_init=2, dt=0.02, seed=1, frame_idx=0, force_iters=0, bank_frame=-1):
        fi = FrameIn()
        fi.current_pose[:] = list(np.asarray(current_pose, np.float64).reshape(12))
        fi.predicted_pose[:] = list(np.asarray(predicted_pose, np.float64).reshape(12))
        fi.prediction[:] = list(np.asarray(prediction, np.float64).reshape(12))
        cm = np.eye(4)[:3].reshape(12) if cam_move_inv is None else np.asarray(cam_move_inv, np.float64).reshape(12)
        fi.cam_move_inv[:] = list(cm)
        keep = None
        if blobs is not None:
            keep = np.ascontiguousarray(blobs, dtype=np.float64).reshape(-1, 2)
            fi.blobs = _dptr(keep)
            fi.B = keep.shape[0]
        else:
            fi.blobs = C.POINTER(C.c_double)()
            fi.B = int(B or 0)
        fi.bank_frame = bank_frame
        fi.it_since_init = it_since_init
        fi.force_iters = force_iters
        fi.dt = dt
        fi.seed = seed
        fi.frame_idx = frame_idx
        fi._keep = keep  # keep the blob buffer alive with the struct
        return fi

    def step(self, frame: FrameIn) -> FrameOut:
        out = FrameOut()
        self._chk(self.lib.pfmpe_step(self.ctx, C.byref(frame), C.byref(out)))
        self._last_out = out
        return out

    def step_batch(self, frames) -> list:
        """Frames (a list of FrameIn) run back to back in C, each blocking on its own record; returns a list."""
        return list(self.run_batch(self.prepare_batch(frames)))

    @staticmethod
    def prepare_batch(frames):
        """The input and output arrays of a step_batch call, built ahead of it (a timed loop then contains only
        the C call: building 20 ctypes frames cost the driver's 20-frame bench line ~1-2 us per frame)."""
        n = len(frames)
        return n, (FrameIn * n)(*frames), (FrameOut * n)()

    def run_batch(self, prepared):
        """pfmpe_step_batch over prepare_batch's arrays; returns prepare_batch's output array itself (a ctypes
        FrameOut array, not a copy): a second run over the same prepared arrays overwrites it (the bench's timed loop
        reuses them on purpose)."""
        n, arr_in, arr_out = prepared
        done = C.c_int()
        self._chk(self.lib.pfmpe_step_batch(self.ctx, arr_in, n, arr_out, C.byref(done)))
        self._last_out = arr_out[n - 1] if n else self._last_out
        return arr_out

    @staticmethod
    def step_multi(engines, frames) -> list:
        """One frame of each engine (independent camera streams / objects) as ONE batch on the device
        (pfmpe_step_multi): frames[s] belongs to engines[s]; outputs and state equal per-engine step()."""
        S = len(engines)
        if S != len(frames) or S == 0:
            raise ValueError("step_multi: one frame per engine")
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        arr_in = (FrameIn * S)(*frames)
        arr_out = (FrameOut * S)()
        engines[0]._chk(engines[0].lib.pfmpe_step_multi(ctxs, S, arr_in, arr_out))
        outs = list(arr_out)
        for e, o in zip(engines, outs):
            e._last_out = o
        return outs

    def step_refine(self, frame: FrameIn, params=None, want_row: bool = False, row=None, cov=None):
        """The step and the Gauss-Newton refinement of its winner in one blocking call (pfmpe_step_refine): what
        step(frame) followed by refine_poses of out.winner_pose / out.corr gives, with one wait.  Returns
        (FrameOut, RefineOut, row, cov): row (a RefineRow) and cov (36 doubles) with want_row, or the caller's own
        `row` / `cov` buffers, which a frame that is not refined leaves as they were; else None."""
        out, gn = FrameOut(), RefineOut()
        if want_row and row is None:
            row = RefineRow()
        if want_row and cov is None:
            cov = np.zeros(36, dtype=np.float64)
        self._chk(self.lib.pfmpe_step_refine(
            self.ctx, C.byref(frame), C.byref(params) if params is not None else None, C.byref(out), C.byref(gn),
            C.byref(row) if row is not None else None, _dptr(cov) if cov is not None else None))
        self._last_out = out
        return out, gn, row, cov

    @staticmethod
    def step_refine_multi(engines, frames, params=None, want_rows: bool = False, rows=None, cov=None):
        """One frame of each engine with its winner's refinement as ONE batch (pfmpe_step_refine_multi): stream s gets
        what engines[s].step_refine(frames[s], params[s]) gives.  params: None, one RefineParams for all, or one per
        engine.  Returns (outs, gns, rows, cov): lists of FrameOut and RefineOut, and with want_rows (or the caller's
        own buffers) a (RefineRow * S) array and an (S, 36) array, else None."""
        S = len(engines)
        if S != len(frames) or S == 0:
            raise ValueError("step_refine_multi: one frame per engine")
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        arr_in = (FrameIn * S)(*frames)
        arr_out, arr_gn = (FrameOut * S)(), (RefineOut * S)()
        ps = None
        if params is not None:
            ps = (RefineParams * S)()
            for s in range(S):
                src = params[s] if isinstance(params, (list, tuple)) else params
                ps[s].max_iter, ps[s].revert_on_divergence, ps[s].converged = (src.max_iter, src.revert_on_divergence,
                                                                               src.converged)
        if want_rows and rows is None:
            rows = (RefineRow * S)()
        if want_rows and cov is None:
            cov = np.zeros((S, 36), dtype=np.float64)
        engines[0]._chk(engines[0].lib.pfmpe_step_refine_multi(
            ctxs, S, arr_in, ps, arr_out, arr_gn, rows, _dptr(cov) if cov is not None else None))
        outs = list(arr_out)
        for e, o in zip(engines, outs):
            e._last_out = o
        return outs, list(arr_gn), rows, cov

    @staticmethod
    def make_roi_in(prediction, predicted_pose, D, image_w, image_h, border, cam_move_inv=None) -> RoiIn:
        """A RoiIn from the arguments of predict_roi (cam_move_inv None: the identity)."""
        ri = RoiIn()
        cm = np.eye(4)[:3].reshape(12) if cam_move_inv is None else np.asarray(cam_move_inv, np.float64).reshape(12)
        ri.cam_move_inv[:] = list(cm)
        ri.prediction[:] = list(np.asarray(prediction, np.float64).reshape(12))
        ri.predicted_pose[:] = list(np.asarray(predicted_pose, np.float64).reshape(12))
        ri.D[:] = list(np.asarray(D, np.float64).reshape(5))
        ri.image_w, ri.image_h, ri.border = int(image_w), int(image_h), int(border)
        return ri

    def predict_roi(self, prediction, predicted_pose, D, image_w, image_h, border, cam_move_inv=None) -> dict:
        """Region of interest for the next detection (PE:396-412): {"roi": [x, y, w, h], "bbox": [...]}."""
        ri = self.make_roi_in(prediction, predicted_pose, D, image_w, image_h, border, cam_move_inv)
        ro = RoiOut()
        self._chk(self.lib.pfmpe_predict_roi(self.ctx, C.byref(ri), C.byref(ro)))
        return _roi_dict(ro)

    @staticmethod
    def predict_roi_multi(engines, ins) -> list:
        """The ROI of one frame of each engine as ONE batch on the device (pfmpe_predict_roi_multi): ins[s] (a RoiIn,
        make_roi_in) belongs to engines[s]; returns one {"roi", "bbox"} per engine, each what predict_roi returns."""
        S = len(engines)
        if S != len(ins) or S == 0:
            raise ValueError("predict_roi_multi: one RoiIn per engine")
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        arr_in = (RoiIn * S)(*ins)
        arr_out = (RoiOut * S)()
        engines[0]._chk(engines[0].lib.pfmpe_predict_roi_multi(ctxs, S, arr_in, arr_out))
        return [_roi_dict(ro) for ro in arr_out]

    def p3p_histogram(self, blobs) -> np.ndarray:
        """Stage 1 of initialise (PE:1526-1716): the B x M correspondence histogram (uint32)."""
        b = np.ascontiguousarray(blobs, dtype=np.float64).reshape(-1, 2)
        h = np.zeros((b.shape[0], self.M), dtype=np.uint32)
        self._chk(self.lib.pfmpe_p3p_histogram(self.ctx, _dptr(b), b.shape[0], h.ctypes.data_as(C.POINTER(C.c_uint32))))
        return h

    def initialise(self, blobs, n_particles=0, certainty_threshold=1.0, valid_corr_threshold=0.5,
                   max_candidates=1 << 20):
        """PoseEstimator::initialise (PE:1503-1786) -> (out dict, histogram).  On success the context's
        particle set is the seeded PoseParticle set (self.N = n_particles)."""
        b = np.ascontiguousarray(blobs, dtype=np.float64).reshape(-1, 2)
        ip = InitParams()
        self.lib.pfmpe_default_init_params(C.byref(ip))
        ip.certainty_threshold = certainty_threshold
        ip.valid_corr_threshold = valid_corr_threshold
        ip.n_particles = int(n_particles)
        ip.max_candidates = int(max_candidates)
        out = InitOut()
        h = np.zeros((b.shape[0], self.M), dtype=np.uint32)
        self._chk(self.lib.pfmpe_initialise(self.ctx, _dptr(b), b.shape[0], C.byref(ip), C.byref(out),
                                            h.ctypes.data_as(C.POINTER(C.c_uint32))))
        d = out.as_dict()
        if d["found"]:
            self.N = int(n_particles) if n_particles else (self.N or self.max_particles)
            self._last_out = None
        return d, h

    @staticmethod
    def initialise_multi(engines, blobs_list, n_particles=0, certainty_threshold=1.0, valid_corr_threshold=0.5,
                         max_candidates=1 << 20, want_hist=True) -> list:
        """PoseEstimator::initialise of every engine as ONE batch on the device (pfmpe_initialise_multi): blobs_list[s]
        belongs to engines[s]; the four parameters are one value for all or one per engine.  Returns one
        (out dict, histogram) per engine, each what engines[s].initialise returns (the histogram is None with
        want_hist=False, and all zeros for a stream with fewer blobs than markers).  A PFError carries the histogram
        arrays as .hist: after a candidate explosion (E_CAP) they hold stage 1's result."""
        S = len(engines)
        if S != len(blobs_list) or S == 0:
            raise ValueError("initialise_multi: one blob list per engine")

        def per(v):
            return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * S

        lib = engines[0].lib
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        bl = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 2) for b in blobs_list]
        ins, ips, outs = (InitIn * S)(), (InitParams * S)(), (InitOut * S)()
        nps = [int(v) for v in per(n_particles)]
        for s in range(S):
            ins[s].blobs = _dptr(bl[s]) if bl[s].shape[0] else C.POINTER(C.c_double)()
            ins[s].B = bl[s].shape[0]
            lib.pfmpe_default_init_params(C.byref(ips[s]))
            ips[s].certainty_threshold = per(certainty_threshold)[s]
            ips[s].valid_corr_threshold = per(valid_corr_threshold)[s]
            ips[s].n_particles = nps[s]
            ips[s].max_candidates = int(per(max_candidates)[s])
        hs = [np.zeros((bl[s].shape[0], engines[s].M), dtype=np.uint32) if want_hist else None for s in range(S)]
        hp = None
        if want_hist:
            hp = (C.POINTER(C.c_uint32) * S)(*[h.ctypes.data_as(C.POINTER(C.c_uint32)) for h in hs])
        try:
            engines[0]._chk(lib.pfmpe_initialise_multi(ctxs, S, ins, ips, outs, hp))
        except PFError as e:
            e.hist = hs  # a candidate explosion (E_CAP after stage 1) leaves stage 1's histograms here
            raise
        res = []
        for s, e in enumerate(engines):
            d = outs[s].as_dict()
            if d["found"]:
                e.N = nps[s] if nps[s] else (e.N or e.max_particles)
                e._last_out = None
            res.append((d, hs[s]))
        return res

    def stage_image(self, image: np.ndarray):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        self._chk(self.lib.pfmpe_stage_image(self.ctx, img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1],
                                             img.shape[0], img.strides[0]))
        self._img_shape = img.shape

    def find_leds(self, image=None, D=None, roi=None, max_out=MAX_BLOBS, **kw):
        """LEDDetector::findLeds (led_detector.cpp:46-215) on the device -> (undistorted B x 2,
        distorted B x 2 float32, info).  image None: the staged image.  kw: DetectParams fields."""
        p = DetectParams()
        self.lib.pfmpe_default_detect_params(C.byref(p))
        if D is not None:
            p.D[:] = list(np.asarray(D, np.float64).reshape(5))
        if roi is not None:
            p.roi_x, p.roi_y, p.roi_w, p.roi_h = [int(v) for v in roi]
        for k, v in kw.items():
            setattr(p, k, v)
        blobs = np.zeros((max(max_out, 1), 2))
        dist = np.zeros((max(max_out, 1), 2), dtype=np.float32)
        out = DetectOut()
        if image is not None:
            img = np.ascontiguousarray(image, dtype=np.uint8)
            ip, (h, w), pitch = img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape, img.strides[0]
        else:
            ip, (h, w) = C.POINTER(C.c_uint8)(), self._img_shape
            pitch = w
        self._chk(self.lib.pfmpe_find_leds(self.ctx, ip, w, h, pitch, C.byref(p), _dptr(blobs),
                                           dist.ctypes.data_as(C.POINTER(C.c_float)), max_out, C.byref(out)))
        n = min(out.n, max_out, MAX_BLOBS)  # the rows the call wrote
        return blobs[:n].copy(), dist[:n].copy(), {"n": out.n, "n_components": out.n_components,
                                                    "overflow": out.overflow}

    def find_leds_multi(self, image=None, rois=(), D=None, params=None, max_out=MAX_BLOBS):
        """pfmpe_find_leds_multi: the ROIs `rois` ((x, y, w, h), or None for the whole image) of one image in one
        launch sequence.  params: a dict of DetectParams fields for every ROI, or a list with one dict per ROI.
        Returns one (undistorted, distorted, info) per ROI, each as find_leds returns it."""
        R = len(rois)
        per_roi = params if isinstance(params, (list, tuple)) else [params or {}] * R
        if len(per_roi) != R:
            raise ValueError("find_leds_multi: one params dict per ROI")
        ps = (DetectParams * max(R, 1))()
        for p, roi, kw in zip(ps, rois, per_roi):
            self.lib.pfmpe_default_detect_params(C.byref(p))
            if D is not None:
                p.D[:] = list(np.asarray(D, np.float64).reshape(5))
            if roi is not None:
                p.roi_x, p.roi_y, p.roi_w, p.roi_h = [int(v) for v in roi]
            for k, v in (kw or {}).items():
                setattr(p, k, v)
        blobs = np.zeros((max(R, 1), max(max_out, 1), 2))
        dist = np.zeros((max(R, 1), max(max_out, 1), 2), dtype=np.float32)
        outs = (DetectOut * max(R, 1))()
        if image is not None:
            img = np.ascontiguousarray(image, dtype=np.uint8)
            ip, (h, w), pitch = img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape, img.strides[0]
        else:
            ip, (h, w) = C.POINTER(C.c_uint8)(), getattr(self, "_img_shape", (0, 0))
            pitch = w
        # the C arrays' ROI stride is 2 * max_out; the numpy rows are max(max_out, 1) wide, the same unless max_out = 0
        self._chk(self.lib.pfmpe_find_leds_multi(self.ctx, ip, w, h, pitch, ps, R, _dptr(blobs),
                                                 dist.ctypes.data_as(C.POINTER(C.c_float)), max_out, outs))
        res = []
        for r in range(R):
            n = min(outs[r].n, max_out, MAX_BLOBS)  # the rows the call wrote
            res.append((blobs[r, :n].copy(), dist[r, :n].copy(),
                        {"n": outs[r].n, "n_components": outs[r].n_components, "overflow": outs[r].overflow}))
        return res

    @staticmethod
    def find_leds_streams(images, image_of, rois, D=None, params=None, max_out=MAX_BLOBS) -> list:
        """pfmpe_find_leds_streams: R detector entries over the images of several cameras in one launch sequence.
        images: a list of (engine, ndarray or None); None is that engine's staged image, and an array's rows may be
        non-contiguous (they are passed with their pitch).  Entry r is the ROI rois[r] ((x, y, w, h), or None for the
        whole image) of images[image_of[r]], with that engine's K.  D: one distortion vector for every entry, or a
        list with one per entry; params: a dict of DetectParams fields for every entry, or a list with one dict per
        entry.  images[0]'s engine leads the batch.  Returns one (undistorted, distorted, info) per entry, each as
        find_leds returns it."""
        R = len(rois)
        if len(images) == 0 or R == 0 or len(image_of) != R:
            raise ValueError("find_leds_streams: at least one image, and one image index per ROI")
        per_roi = params if isinstance(params, (list, tuple)) else [params or {}] * R
        if len(per_roi) != R:
            raise ValueError("find_leds_streams: one params dict per ROI")
        per_d = [D] * R if D is None or np.ndim(D) == 1 else list(D)
        if len(per_d) != R:
            raise ValueError("find_leds_streams: one D per ROI")
        lead = images[0][0]
        ims, keep = make_detect_images([(e.ctx, img, getattr(e, "_img_shape", None)) for e, img in images])
        ps = make_detect_params(rois, per_d, per_roi)
        idx = (C.c_int32 * R)(*[int(i) for i in image_of])
        blobs = np.zeros((R, max(max_out, 1), 2))
        dist = np.zeros((R, max(max_out, 1), 2), dtype=np.float32)
        outs = (DetectOut * R)()
        lead._chk(lead.lib.pfmpe_find_leds_streams(ims, len(images), idx, ps, R, _dptr(blobs),
                                                   dist.ctypes.data_as(C.POINTER(C.c_float)), max_out, outs))
        del keep
        res = []
        for r in range(R):
            n = min(outs[r].n, max_out, MAX_BLOBS)  # the rows the call wrote
            res.append((blobs[r, :n].copy(), dist[r, :n].copy(),
                        {"n": outs[r].n, "n_components": outs[r].n_components, "overflow": outs[r].overflow}))
        return res

    def stage_blob_stream(self, path) -> int:
        """Stage every frame of a PFMB stream file in the device blob bank; returns the frame count."""
        n = C.c_int()
        self._chk(self.lib.pfmpe_stage_blob_stream(self.ctx, _enc(path), C.byref(n)))
        return n.value

    def get_particles(self, which: int) -> np.ndarray:
        out = np.empty((self.N, 12), dtype=np.float64)
        self._chk(self.lib.pfmpe_get_particles(self.ctx, which, _dptr(out)))
        return out

    def get_weights(self) -> np.ndarray:
        out = np.empty(self.N, dtype=np.float64)
        self._chk(self.lib.pfmpe_get_weights(self.ctx, _dptr(out)))
        return out

    def get_counts(self) -> np.ndarray:
        out = np.empty(self.N, dtype=np.uint32)
        self._chk(self.lib.pfmpe_get_counts(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def cloud_stats(self, which: int = CLOUD_POSTERIOR, ref=None) -> dict:
        """Mean twist, 6x6 covariance ([upsilon; omega], left perturbation of `ref`), ESS, mean pose and extent of
        the particle cloud, reduced on the device (pfmpe_cloud_stats).  which: CLOUD_POSTERIOR (the current prior,
        unit weights) or CLOUD_WEIGHTED (the last step's kept propagated set with its raw weights).  ref None: the
        last step's winner_pose when it resampled, else its most_likely_pose; before any step a ref is required."""
        if ref is None:
            lo = self._last_out
            if lo is None:
                raise ValueError("cloud_stats: no step yet on this particle set, pass ref")
            ref = lo.winner_pose if lo.resampled else lo.most_likely_pose
        r = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(-1)[:12])
        if r.size != 12:
            raise ValueError("cloud_stats: ref must hold 12 values (3x4) or a 4x4")
        out = CloudOut()
        self._chk(self.lib.pfmpe_cloud_stats(self.ctx, int(which), _dptr(r), C.byref(out)))
        return out.as_dict()

    @staticmethod
    def make_cloud_in(which: int, ref) -> CloudIn:
        """A CloudIn from the arguments of cloud_stats (ref: 12 values, 3x4 or 4x4; no default)."""
        r = np.asarray(ref, dtype=np.float64).reshape(-1)[:12]
        if r.size != 12:
            raise ValueError("cloud_stats_multi: ref must hold 12 values (3x4) or a 4x4")
        ci = CloudIn()
        ci.ref_pose[:] = r.tolist()
        ci.which = int(which)
        return ci

    @staticmethod
    def cloud_stats_multi(engines, whichs, refs) -> list:
        """The cloud statistics of S entries as ONE batch on the device (pfmpe_cloud_stats_multi): entry s is
        cloud_stats(whichs[s], refs[s]) of engines[s] (an engine may appear several times: both sets of one object, or
        two reference poses); returns one dict per entry, each what cloud_stats returns."""
        S = len(engines)
        if S == 0 or S != len(whichs) or S != len(refs):
            raise ValueError("cloud_stats_multi: one which and one ref per engine")
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        arr_in = (CloudIn * S)(*[Engine.make_cloud_in(w, r) for w, r in zip(whichs, refs)])
        arr_out = (CloudOut * S)()
        engines[0]._chk(engines[0].lib.pfmpe_cloud_stats_multi(ctxs, S, arr_in, arr_out))
        return [o.as_dict() for o in arr_out]

    def cloud_modes(self, which: int, seeds, params=None, trans_scale=None, rot_scale=None, max_dist=None,
                    want_mode_of: bool = True) -> tuple:
        """The cloud's mass and statistics per hypothesis (pfmpe_cloud_modes): every particle of the set `which` goes
        to the nearest of the K seeds (K x 12, or K 3x4 / 4x4 poses; from top_particles or the caller's).  Returns
        (K + 1 dicts, mode_of): dict k is what cloud_stats returns for the members of mode k about seed k, with
        "share", its part of the total weight; dict K describes the particles no seed takes (about seed 0).  mode_of:
        every particle's mode (uint8, MODE_NONE for none), or None with want_mode_of false (nothing per particle
        crosses the host link then).  params: a ModesParams, default pfmpe_default_modes_params; the keyword scales
        override its fields."""
        sd, prm = _modes_args(seeds, params, trans_scale, rot_scale, max_dist)
        K = sd.shape[0]
        out = (ModeOut * (K + 1))()
        mode_of = np.empty(self.N, dtype=np.uint8) if want_mode_of else None
        self._chk(self.lib.pfmpe_cloud_modes(
            self.ctx, int(which), _dptr(sd), K, C.byref(prm), out,
            mode_of.ctypes.data_as(C.POINTER(C.c_uint8)) if want_mode_of else None))
        return [o.as_dict() for o in out], mode_of

    def resample_prior(self, n_new: int, src=None, seeds=None, mode: int = 0, trans_scale=None, rot_scale=None,
                       max_dist: float = 0.0) -> dict:
        """A new prior of n_new particles for this engine from the members of src's prior (src None: this engine's own,
        in place), gathered on the device (pfmpe_resample_prior).  seeds None: every particle is a member; else the
        members are the particles cloud_modes(CLOUD_POSTERIOR, seeds, ...) gives `mode` (0 .. K-1, or MODE_NONE), with
        the same scales and gate (defaults: pfmpe_default_modes_params).  Returns {"n_src", "n_members", "n_new"};
        n_new is 0, and this engine unchanged, when the mode has no member."""
        src = self if src is None else src
        prm = ResampleParams()
        prm.n_new = int(n_new)
        if seeds is not None:
            sd, prm.modes = _modes_args(seeds, None, trans_scale, rot_scale, max_dist)
            prm.K, prm.seeds, prm.mode = sd.shape[0], _dptr(sd), int(mode)
        out = ResampleOut()
        self._chk(self.lib.pfmpe_resample_prior(self.ctx, src.ctx, C.byref(prm), C.byref(out)))
        if out.n_new > 0:
            self.N = int(out.n_new)
            self._last_out = None
        return out.as_dict()

    @staticmethod
    def _assoc_in(blobs, bank_frame):
        ai = AssocIn()
        keep = None
        if blobs is not None and bank_frame < 0:
            keep = np.ascontiguousarray(blobs, dtype=np.float64).reshape(-1, 2)
            ai.blobs = _dptr(keep)
            ai.B = keep.shape[0]
        ai.bank_frame = int(bank_frame)
        return ai, keep

    def assoc_stats(self, which: int = ASSOC_POSTERIOR, blobs=None, bank_frame: int = -1, want_votes: bool = True) -> dict:
        """Which blob each LED matched, counted over a particle set on the device (pfmpe_assoc_stats).  which:
        ASSOC_POSTERIOR (the current prior) or ASSOC_PROPAGATED (the last step's kept propagated set); blobs: the
        frame's B x 2 list, or bank_frame: a frame of the staged bank.  Returns AssocOut.as_dict() plus, with
        want_votes, "votes": the (M, B + 1) uint32 table (column 0: particles that left the LED unpaired)."""
        ai, keep = self._assoc_in(blobs, bank_frame)
        out = AssocOut()
        votes = None
        vp = C.POINTER(C.c_uint32)()
        if want_votes:
            nb = keep.shape[0] if keep is not None else 0
            if bank_frame >= 0:  # the frame's count comes back in out.B: room for the largest frame
                nb = MAX_BLOBS
            votes = np.zeros(max(self.M, 1) * (nb + 1), dtype=np.uint32)
            vp = votes.ctypes.data_as(C.POINTER(C.c_uint32))
        self._chk(self.lib.pfmpe_assoc_stats(self.ctx, int(which), C.byref(ai), C.byref(out), vp))
        d = out.as_dict()
        if want_votes:
            d["votes"] = votes[: out.M * (out.B + 1)].reshape(out.M, out.B + 1).copy()
        return d

    @staticmethod
    def assoc_stats_multi(engines, whichs, blobs_list=None, bank_frames=None, want_votes: bool = True) -> list:
        """The association votes of S entries as ONE batch on the device (pfmpe_assoc_stats_multi): entry s is
        assoc_stats(whichs[s], blobs_list[s] or bank_frames[s]) of engines[s] (an engine may appear several times: both
        sets of one object, or two blob lists; a bank frame is one of ITS engine's staged bank).  Returns one dict per
        entry, each what assoc_stats returns."""
        S = len(engines)
        blobs_list = [None] * S if blobs_list is None else list(blobs_list)
        bank_frames = [-1] * S if bank_frames is None else list(bank_frames)
        if S == 0 or S != len(whichs) or S != len(blobs_list) or S != len(bank_frames):
            raise ValueError("assoc_stats_multi: one which and one blob list or bank frame per engine")
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        arr_in = (AssocMultiIn * S)()
        keep, tabs = [], []
        vps = (C.POINTER(C.c_uint32) * S)()
        for s in range(S):
            ai, kb = Engine._assoc_in(blobs_list[s], int(bank_frames[s]))
            keep.append(kb)
            arr_in[s].blobs = ai
            arr_in[s].which = int(whichs[s])
            if want_votes:  # a bank frame's count comes back in out.B: room for the largest frame
                nb = MAX_BLOBS if int(bank_frames[s]) >= 0 else (kb.shape[0] if kb is not None else 0)
                tabs.append(np.zeros(max(engines[s].M, 1) * (nb + 1), dtype=np.uint32))
                vps[s] = tabs[s].ctypes.data_as(C.POINTER(C.c_uint32))
        arr_out = (AssocOut * S)()
        engines[0]._chk(engines[0].lib.pfmpe_assoc_stats_multi(ctxs, S, arr_in, arr_out, vps if want_votes else None))
        res = []
        for s, o in enumerate(arr_out):
            d = o.as_dict()
            if want_votes:
                d["votes"] = tabs[s][: o.M * (o.B + 1)].reshape(o.M, o.B + 1).copy()
            res.append(d)
        return res

    def get_pairs(self, which: int, blobs=None, bank_frame: int = -1, first: int = 0, count=None):
        """The pairs of particles first .. first + count - 1 of a set (pfmpe_get_pairs; count None: to the end):
        (corr[count, MAX_MARKERS, 2] uint32 of 1-based (LED, blob) rows padded with zeros, n_corr[count] int32)."""
        ai, keep = self._assoc_in(blobs, bank_frame)
        if count is None:
            count = self.N - int(first)
        n = max(int(count), 0)
        corr = np.zeros((n, MAX_MARKERS, 2), dtype=np.uint32)
        n_corr = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.pfmpe_get_pairs(self.ctx, int(which), C.byref(ai), int(first), int(count),
                                           corr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           n_corr.ctypes.data_as(C.POINTER(C.c_int32))))
        return corr, n_corr

    def top_particles(self, key: int = TOP_BY_WEIGHT, K: int = 8, min_trans: float = 0.0, min_rot: float = 0.0,
                      blobs=None, bank_frame: int = -1) -> dict:
        """The K best distinct hypotheses of the last step's kept propagated set, ranked on the device
        (pfmpe_top_particles).  key: TOP_BY_WEIGHT (the raw weights of get_weights) or TOP_BY_COUNT (get_counts);
        min_trans (m) / min_rot (rad): a candidate closer than both to a better kept one is dropped (0: that threshold
        does not separate; both 0: the plain ranking).  blobs / bank_frame: also each row's pairs.  Returns
        TopOut.as_dict() plus the n_out rows: "index" int32, "key_value" and "poses" (n_out, 12) float64 and, with
        blobs, "corr" (n_out, MAX_MARKERS, 2) uint32 and "n_corr" int32, ready for refine_poses."""
        prm = TopParams(int(key), int(K), float(min_trans), float(min_rot))
        want_pairs = blobs is not None or bank_frame >= 0
        ai, keep = self._assoc_in(blobs, bank_frame)
        k = min(max(int(K), 0), TOP_MAX)
        index = np.zeros(k, dtype=np.int32)
        key_value = np.zeros(k, dtype=np.float64)
        poses = np.zeros((k, 12), dtype=np.float64)
        corr = np.zeros((k, MAX_MARKERS, 2), dtype=np.uint32)
        n_corr = np.zeros(k, dtype=np.int32)
        out = TopOut()
        self._chk(self.lib.pfmpe_top_particles(
            self.ctx, C.byref(prm), C.byref(ai) if want_pairs else None, C.byref(out),
            index.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(key_value), _dptr(poses),
            corr.ctypes.data_as(C.POINTER(C.c_uint32)) if want_pairs else None,
            n_corr.ctypes.data_as(C.POINTER(C.c_int32)) if want_pairs else None))
        d = out.as_dict()
        n = out.n_out
        d.update(index=index[:n], key_value=key_value[:n], poses=poses[:n])
        if want_pairs:
            d.update(corr=corr[:n], n_corr=n_corr[:n])
        return d

    def _refine_result(self, out, rows, cov):
        d = out.as_dict()
        d["rows"] = rows
        if cov is not None:
            d["cov"] = cov
        return d

    def refine_poses(self, poses, pairs, blobs=None, bank_frame: int = -1, params=None, want_cov: bool = False) -> dict:
        """Gauss-Newton (optimisePose) of K hypotheses on the device (pfmpe_refine_poses).  poses: K x 12 (or K 3x4 /
        4x4 matrices); pairs: K x MAX_MARKERS x 2 1-based (LED, blob) rows padded with zeros (FrameOut.corr, get_pairs);
        blobs: the frame's B x 2 list, or bank_frame.  Returns the summary (RefineOut.as_dict()) plus "rows", a
        REFINE_ROW_DTYPE array of K records, and with want_cov "cov" (K, 6, 6)."""
        ai, keep = self._assoc_in(blobs, bank_frame)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, MAX_MARKERS, 2)
        k = pairs.shape[0]
        poses = np.asarray(poses, dtype=np.float64)
        if poses.shape[-2:] == (4, 4):
            poses = poses[..., :3, :]
        poses = np.ascontiguousarray(poses.reshape(-1, 12))
        if poses.shape[0] != k:
            raise ValueError("refine_poses: one pair table per pose")
        rows = np.zeros(k, dtype=REFINE_ROW_DTYPE)
        cov = np.zeros((k, 6, 6), dtype=np.float64) if want_cov else None
        out = RefineOut()
        self._chk(self.lib.pfmpe_refine_poses(
            self.ctx, C.byref(ai), C.byref(params) if params is not None else None, _dptr(poses),
            pairs.ctypes.data_as(C.POINTER(C.c_uint32)), k, C.byref(out), rows.ctypes.data_as(C.c_void_p),
            _dptr(cov) if want_cov else None))
        return self._refine_result(out, rows, cov)

    def refine_cloud(self, which: int, blobs=None, bank_frame: int = -1, first: int = 0, count=None, params=None,
                     want_cov: bool = False) -> dict:
        """Gauss-Newton of every particle of a set from its own pairs (pfmpe_refine_cloud).  The summary covers all N
        particles; "rows" (and "cov" with want_cov) cover particles first .. first + count - 1 (count None: to the
        end; count 0: the summary alone)."""
        ai, keep = self._assoc_in(blobs, bank_frame)
        if count is None:
            count = self.N - int(first)
        n = max(int(count), 0)
        rows = np.zeros(n, dtype=REFINE_ROW_DTYPE)
        cov = np.zeros((n, 6, 6), dtype=np.float64) if want_cov else None
        out = RefineOut()
        self._chk(self.lib.pfmpe_refine_cloud(
            self.ctx, int(which), C.byref(ai), C.byref(params) if params is not None else None, int(first), int(count),
            C.byref(out), rows.ctypes.data_as(C.c_void_p) if n else None, _dptr(cov) if (want_cov and n) else None))
        return self._refine_result(out, rows, cov)

    @staticmethod
    def refine_multi(engines, poses_list, pairs_list, blobs_list=None, bank_frames=None, params=None,
                     want_rows: bool = True, want_cov: bool = False) -> list:
        """Gauss-Newton of the hypotheses of every engine as ONE batch on the device (pfmpe_refine_multi): poses_list[s]
        (K_s x 12, K_s may be 0) and pairs_list[s] (K_s x MAX_MARKERS x 2) belong to engines[s], with the blob list
        blobs_list[s] or the frame bank_frames[s] (>= 0) of that engine's staged bank.  An engine may appear more than
        once.  params: None (the defaults), one RefineParams for all, or one per engine.  Returns one dict per stream
        in the shape refine_poses returns ("rows" with want_rows, "cov" with want_cov)."""
        S = len(engines)
        if S == 0 or S != len(poses_list) or S != len(pairs_list):
            raise ValueError("refine_multi: one pose set and one pair set per engine")
        if blobs_list is None:
            blobs_list = [None] * S
        if bank_frames is None:
            bank_frames = [-1] * S
        if len(blobs_list) != S or len(bank_frames) != S:
            raise ValueError("refine_multi: one blob list / bank frame per engine")
        lib = engines[0].lib
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engines])
        ins, outs = (RefineIn * S)(), (RefineOut * S)()
        keep, rows, covs = [], [], []
        for s in range(S):
            ai, kb = Engine._assoc_in(blobs_list[s], int(bank_frames[s]))
            pr = np.ascontiguousarray(pairs_list[s], dtype=np.uint32).reshape(-1, MAX_MARKERS, 2)
            k = pr.shape[0]
            po = np.asarray(poses_list[s], dtype=np.float64)
            if po.shape[-2:] == (4, 4):
                po = po[..., :3, :]
            po = np.ascontiguousarray(po.reshape(-1, 12))
            if po.shape[0] != k:
                raise ValueError("refine_multi: one pair table per pose")
            keep.append((kb, pr, po))
            ins[s].blobs = ai
            ins[s].poses = _dptr(po) if k else C.POINTER(C.c_double)()
            ins[s].corr = pr.ctypes.data_as(C.POINTER(C.c_uint32)) if k else C.POINTER(C.c_uint32)()
            ins[s].K = k
            rows.append(np.zeros(k, dtype=REFINE_ROW_DTYPE) if want_rows else None)
            covs.append(np.zeros((k, 6, 6), dtype=np.float64) if want_cov else None)
        ps = None
        if params is not None:
            ps = (RefineParams * S)()
            for s in range(S):
                src = params[s] if isinstance(params, (list, tuple)) else params
                ps[s].max_iter, ps[s].revert_on_divergence, ps[s].converged = (src.max_iter, src.revert_on_divergence,
                                                                               src.converged)
        rp = (C.c_void_p * S)(*[r.ctypes.data if (r is not None and len(r)) else None for r in rows]) if want_rows else None
        cp = None
        if want_cov:
            cp = (C.POINTER(C.c_double) * S)(*[_dptr(c) if len(c) else C.POINTER(C.c_double)() for c in covs])
        engines[0]._chk(lib.pfmpe_refine_multi(ctxs, S, ins, ps, outs, rp, cp))
        res = []
        for s in range(S):
            d = outs[s].as_dict()
            if want_rows:
                d["rows"] = rows[s]
            if want_cov:
                d["cov"] = covs[s]
            res.append(d)
        return res

    def kernel_stats(self) -> dict:
        res = {}
        for k in range(K_COUNT):
            n = C.c_int64()
            ms = C.c_double()
            self._chk(self.lib.pfmpe_get_kernel_stats(self.ctx, k, C.byref(n), C.byref(ms)))
            res[self.lib.pfmpe_kernel_name(k).decode()] = (n.value, ms.value)
        return res

    def reset_kernel_stats(self):
        self._chk(self.lib.pfmpe_reset_kernel_stats(self.ctx))


def _enc(x):
    return x.encode() if isinstance(x, str) else x


def _roi_dict(ro: RoiOut) -> dict:
    return {"roi": [ro.x, ro.y, ro.width, ro.height], "bbox": np.array(list(ro.bbox))}


def host_predict_roi(markers, K, poses, roi_in: RoiIn) -> dict:
    """predict_roi on the host for caller-given poses (pfmpe_host_predict_roi: the code a lane of the ROI kernels
    runs, then the same host end).  poses: N x 12 (N may be 0: the markers at predicted_pose_ only)."""
    m = np.ascontiguousarray(markers, dtype=np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(K, dtype=np.float64).reshape(-1)
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    if k.size != 9:
        raise ValueError("host_predict_roi: K must be 3x3")
    ro = RoiOut()
    rc = load().pfmpe_host_predict_roi(_dptr(m), m.shape[0], _dptr(k), _dptr(p) if p.shape[0] else None, p.shape[0],
                                       C.byref(roi_in), C.byref(ro))
    if rc != OK:
        raise PFError(rc, "host_predict_roi: 1 <= M <= %d markers and image sides >= 1" % MAX_MARKERS)
    return _roi_dict(ro)


def parse_marker_yaml(text) -> np.ndarray:
    """Marker positions (M x 3) from the reference's marker YAML (README.md:95-117)."""
    lib = load()
    n = lib.pfmpe_parse_marker_yaml(_enc(text), None, 0)
    if n < 0:
        raise PFError(n, "malformed marker YAML")
    out = np.zeros((n, 3))
    lib.pfmpe_parse_marker_yaml(_enc(text), _dptr(out), n)
    return out


def parse_launch(text) -> LaunchConfig:
    """PF / init / marker-split parameters of a ROS launch file (pf_mpe/launch/<name>.launch)."""
    lib = load()
    cfg = LaunchConfig()
    lib.pfmpe_default_launch_config(C.byref(cfg))
    n = lib.pfmpe_parse_launch(_enc(text), C.byref(cfg))
    if n < 0:
        raise PFError(n, "malformed launch text")
    cfg.n_known = n
    return cfg


def parse_camera_info(text) -> dict:
    """K (3x3), D (5), width, height from a sensor_msgs/CameraInfo echo (README.md:127-143)."""
    K = np.zeros(9)
    D = np.zeros(5)
    w, h = C.c_int32(), C.c_int32()
    m = load().pfmpe_parse_camera_info(_enc(text), _dptr(K), _dptr(D), C.byref(w), C.byref(h))
    if m < 0:
        raise PFError(m, "malformed camera_info")
    return {"K": K.reshape(3, 3), "D": D, "width": w.value, "height": h.value, "found": m}


def write_blob_stream(path, frames, timestamps=None):
    """Recorded detections (a list of B_f x 2 arrays, undistorted px) -> the PFMB stream file."""
    offs = np.zeros(len(frames) + 1, dtype=np.int32)
    for i, f in enumerate(frames):
        offs[i + 1] = offs[i] + len(f)
    allb = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float64).reshape(-1, 2) for f in frames]
                                               + [np.zeros((0, 2))]), dtype=np.float64)
    ts = np.ascontiguousarray(np.zeros(len(frames)) if timestamps is None else timestamps, dtype=np.float64)
    rc = load().pfmpe_write_blob_stream(_enc(path), _dptr(ts), _dptr(allb), offs.ctypes.data_as(C.POINTER(C.c_int32)),
                                        len(frames))
    if rc != OK:
        raise PFError(rc, f"cannot write {path}")


def read_blob_stream(path):
    """PFMB stream file -> (timestamps, list of B_f x 2 arrays)."""
    lib = load()
    nf, nb = C.c_int(), C.c_int64()
    rc = lib.pfmpe_read_blob_stream(_enc(path), None, None, None, 0, 0, C.byref(nf), C.byref(nb))
    if rc != OK:
        raise PFError(rc, f"cannot read {path}")
    ts = np.zeros(nf.value)
    bl = np.zeros((max(nb.value, 1), 2))
    off = np.zeros(nf.value + 1, dtype=np.int32)
    rc = lib.pfmpe_read_blob_stream(_enc(path), _dptr(ts), _dptr(bl), off.ctypes.data_as(C.POINTER(C.c_int32)), nf.value,
                                    nb.value, C.byref(nf), C.byref(nb))
    if rc != OK:
        raise PFError(rc, f"cannot read {path}")
    return ts, [bl[off[i]:off[i + 1]].copy() for i in range(nf.value)]


def host_ref_uniform(seed: int, j: int, a: float, b: float) -> float:
    return load().pfmpe_host_ref_uniform(seed, j, a, b)


def host_pose_twist(pose, ref) -> np.ndarray:
    """Twist [upsilon; omega] of pose * ref^-1 (poses: 12 values, or 4x4), by the code the cloud kernel runs."""
    p = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(-1)[:12])
    r = np.ascontiguousarray(np.asarray(ref, dtype=np.float64).reshape(-1)[:12])
    out = np.zeros(6)
    load().pfmpe_host_pose_twist(_dptr(p), _dptr(r), _dptr(out))
    return out


def default_refine_params() -> RefineParams:
    p = RefineParams()
    load().pfmpe_default_refine_params(C.byref(p))
    return p


def host_optimise_pose(markers, K, blobs, pairs, pose, params=None):
    """optimisePose of one hypothesis on the host (pfmpe_host_optimise_pose: the code a lane of k_refine runs).  pairs:
    (n, 2) 1-based (LED, blob) rows, blob 0 rows skipped.  Returns (row, cov): a REFINE_ROW_DTYPE record and (6, 6)."""
    m = np.ascontiguousarray(markers, dtype=np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(K, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(blobs, dtype=np.float64).reshape(-1, 2)
    c = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    p = np.asarray(pose, dtype=np.float64)
    if p.shape == (4, 4):
        p = p[:3, :]
    p = np.ascontiguousarray(p.reshape(-1))
    if k.size != 9 or p.size != 12:
        raise ValueError("host_optimise_pose: K must be 3x3 and pose 3x4 (or 4x4)")
    row = RefineRow()
    cov = np.zeros((6, 6), dtype=np.float64)
    rc = load().pfmpe_host_optimise_pose(_dptr(m), m.shape[0], _dptr(k), _dptr(b), b.shape[0],
                                         c.ctypes.data_as(C.POINTER(C.c_uint32)), c.shape[0],
                                         C.byref(params) if params is not None else None, _dptr(p), C.byref(row), _dptr(cov))
    if rc != OK:
        raise PFError(rc, "host_optimise_pose: bad arguments")
    return np.frombuffer(bytes(row), dtype=REFINE_ROW_DTYPE)[0].copy(), cov


def host_step_tail(markers, K, blobs, frame: FrameOut, params=None, row=None, cov=None):
    """The step's tail on the host (pfmpe_host_step_tail; no GPU): what step_refine publishes for the finished frame
    `frame` against the blob list `blobs`.  Returns (RefineOut, row, cov); the caller's own `row` / `cov` buffers are
    left as they were when the frame is not refined."""
    m = np.ascontiguousarray(markers, dtype=np.float64).reshape(-1, 3)
    k = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    b = np.ascontiguousarray(blobs if blobs is not None else np.zeros((0, 2)), dtype=np.float64).reshape(-1, 2)
    gn = RefineOut()
    row = RefineRow() if row is None else row
    cov = np.zeros(36, dtype=np.float64) if cov is None else cov
    rc = load().pfmpe_host_step_tail(_dptr(m), m.shape[0], _dptr(k), _dptr(b) if b.shape[0] else None, b.shape[0],
                                     C.byref(frame), C.byref(params) if params is not None else None, C.byref(gn),
                                     C.byref(row), _dptr(cov))
    if rc != OK:
        raise PFError(rc, "pfmpe_host_step_tail: bad arguments")
    return gn, row, cov


def host_assoc_summary(votes) -> dict:
    """n, matched and the mode / runner-up fields of an (M, B + 1) votes table (pfmpe_host_assoc_summary, the code
    assoc_stats runs after its read-back); ValueError when the rows do not all sum to the same n."""
    v = np.ascontiguousarray(votes, dtype=np.uint32)
    if v.ndim != 2 or v.shape[1] < 1:
        raise ValueError("host_assoc_summary: votes must be an (M, B + 1) table")
    out = AssocOut()
    rc = load().pfmpe_host_assoc_summary(v.ctypes.data_as(C.POINTER(C.c_uint32)), v.shape[0], v.shape[1] - 1,
                                         C.byref(out))
    if rc != OK:
        raise PFError(rc, "host_assoc_summary: bad table (rows must sum to one n, 1 <= M <= %d)" % MAX_MARKERS)
    d = out.as_dict()
    del d["n_any"], d["npairs_hist"]
    return d


def host_assoc_plan(N, M, B, which=None, prune=None, table_bytes=None, state_dtype: int = STATE_F32) -> tuple:
    """pfmpe_host_assoc_plan: the layout of an assoc_stats_multi batch whose entry s has N[s] particles, M[s] LEDs and
    B[s] blobs (which / prune / table_bytes: per entry, or None for all POSTERIOR / all pruned / tables without a
    grid).  Returns (one dict per entry: bins_offset, first_block, blocks, launch, lds_votes; the totals' dict)."""
    arrs = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) if a is not None else None
            for a in (N, M, B, which, prune, table_bytes)]
    S = arrs[0].size
    if any(a is not None and a.size != S for a in arrs):
        raise ValueError("host_assoc_plan: one value per entry in every array")
    plan = (AssocPlan * max(S, 1))()
    total = AssocPlanTotal()
    ptr = [a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None for a in arrs]
    rc = load().pfmpe_host_assoc_plan(*ptr, S, int(state_dtype), plan, C.byref(total))
    if rc != OK:
        raise PFError(rc, "pfmpe_host_assoc_plan")
    return [plan[s].as_dict() for s in range(S)], total.as_dict()


def default_gate_params() -> GateParams:
    p = GateParams()
    load().pfmpe_default_gate_params(C.byref(p))
    return p


def host_gate_pairs(votes, pairs, n_corr=None, params=None, min_share=None, lead=None, min_pairs=None) -> dict:
    """pfmpe_host_gate_pairs: the pairs of a row (pairs: up to MAX_MARKERS 1-based (LED, blob) rows, e.g.
    FrameOut.pairs(); n_corr None: all of them) that an (M, B + 1) votes table supports.  params: a GateParams, default
    pfmpe_default_gate_params (0.5, 2.0, 4); the keywords override its fields.  Returns n_in, n_gated, fallback,
    reason (n_in uint8: bit 0 too little support, bit 1 not the LED's mode, bit 2 a contested mode) and gated, the
    (MAX_MARKERS, 2) uint32 row to refine: the kept pairs, or with fallback the input row."""
    v = np.ascontiguousarray(votes, dtype=np.uint32)
    if v.ndim != 2 or v.shape[1] < 1:
        raise ValueError("host_gate_pairs: votes must be an (M, B + 1) table")
    pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    n = pr.shape[0] if n_corr is None else int(n_corr)
    row = np.zeros((MAX_MARKERS, 2), dtype=np.uint32)
    m = min(pr.shape[0], MAX_MARKERS)
    row[:m] = pr[:m]
    prm = GateParams()
    C.memmove(C.byref(prm), C.byref(params if params is not None else default_gate_params()), C.sizeof(GateParams))
    for k, val in (("min_share", min_share), ("lead", lead), ("min_pairs", min_pairs)):
        if val is not None:
            setattr(prm, k, val)
    gated = np.zeros((MAX_MARKERS, 2), dtype=np.uint32)
    out = GateOut()
    u32 = C.POINTER(C.c_uint32)
    rc = load().pfmpe_host_gate_pairs(v.ctypes.data_as(u32), v.shape[0], v.shape[1] - 1, row.ctypes.data_as(u32), n,
                                      C.byref(prm), gated.ctypes.data_as(u32), C.byref(out))
    if rc != OK:
        raise PFError(rc, "pfmpe_host_gate_pairs: bad table, row or parameters")
    return {"n_in": out.n_in, "n_gated": out.n_gated, "fallback": out.fallback,
            "reason": np.array(out.reason[: out.n_in], dtype=np.uint8), "gated": gated}


def default_top_params() -> TopParams:
    p = TopParams()
    load().pfmpe_default_top_params(C.byref(p))
    return p


def host_top_suppress(poses, K: int, min_trans: float = 0.0, min_rot: float = 0.0) -> dict:
    """The suppression walk of top_particles on the host (pfmpe_host_top_suppress), for P poses already in rank order
    (P x 12, any P): "keep" the positions kept (n_out of them), "n_out", "n_examined"."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    keep = np.zeros(max(int(K), 1), dtype=np.int32)
    n_out, n_ex = C.c_int32(-1), C.c_int32(-1)
    rc = load().pfmpe_host_top_suppress(_dptr(p), p.shape[0], int(K), float(min_trans), float(min_rot),
                                        keep.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out), C.byref(n_ex))
    if rc != OK:
        raise PFError(rc, "host_top_suppress: bad arguments")
    return {"keep": keep[: n_out.value].copy(), "n_out": n_out.value, "n_examined": n_ex.value}


def default_modes_params() -> ModesParams:
    p = ModesParams()
    load().pfmpe_default_modes_params(C.byref(p))
    return p


def _modes_args(seeds, params, trans_scale, rot_scale, max_dist):
    """The seeds as a K x 12 array and a ModesParams of its own (params, or the defaults, with the overrides)."""
    sd = np.asarray(seeds, dtype=np.float64)
    if sd.ndim >= 2 and sd.shape[-2:] == (4, 4):
        sd = sd.reshape(-1, 4, 4)[:, :3, :]
    sd = np.ascontiguousarray(sd.reshape(-1, 12))
    src = params if params is not None else default_modes_params()
    prm = ModesParams(src.trans_scale, src.rot_scale, src.max_dist)
    for name, v in (("trans_scale", trans_scale), ("rot_scale", rot_scale), ("max_dist", max_dist)):
        if v is not None:
            setattr(prm, name, float(v))
    return sd, prm


def host_cloud_assign(poses, seeds, params=None, trans_scale=None, rot_scale=None, max_dist=None) -> tuple:
    """The assignment of cloud_modes on the host (pfmpe_host_cloud_assign), by the function the device runs, for N
    poses (N x 12, any N): (mode_of (N uint8), counts (K + 1 int64: modes 0 .. K-1, then the particles without one))."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    sd, prm = _modes_args(seeds, params, trans_scale, rot_scale, max_dist)
    K = sd.shape[0]
    mode_of = np.empty(max(p.shape[0], 1), dtype=np.uint8)
    counts = np.zeros(max(K, 0) + 1, dtype=np.int64)
    rc = load().pfmpe_host_cloud_assign(_dptr(p), p.shape[0], _dptr(sd), K, C.byref(prm),
                                        mode_of.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        counts.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != OK:
        raise PFError(rc, "host_cloud_assign: bad arguments")
    return mode_of[: p.shape[0]], counts


def host_resample_source(mode_of, mode: int, n_new: int, N=None) -> tuple:
    """The source particle of every slot of a new prior of n_new particles (pfmpe_host_resample_source), by the rule
    pfmpe_resample_prior runs: (source (int32, n_new entries; none when there is no member), n_members).  mode_of: every
    particle's mode (uint8), the members being those equal to `mode`; None with N: all N particles are members."""
    mo = None if mode_of is None else np.ascontiguousarray(mode_of, dtype=np.uint8)
    n = int(N) if mo is None else mo.shape[0]
    source = np.empty(max(int(n_new), 1), dtype=np.int32)
    m = C.c_int64(-1)
    rc = load().pfmpe_host_resample_source(None if mo is None else mo.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(mode),
                                           int(n_new), source.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(m))
    if rc != OK:
        raise PFError(rc, "host_resample_source: bad arguments")
    return source[: int(n_new) if m.value > 0 else 0].copy(), m.value


def host_resample_rank(k: int, m: int, n_new: int) -> int:
    """The rank of the member slot k of n_new copies, of m members (pfmpe_host_resample_rank)."""
    r = C.c_int64(-1)
    rc = load().pfmpe_host_resample_rank(int(k), int(m), int(n_new), C.byref(r))
    if rc != OK:
        raise PFError(rc, "host_resample_rank: bad arguments")
    return r.value


def make_detect_images(images):
    """A DetectImage array from (ctx or None, ndarray or None, staged (h, w) or None) triples -> (array, the arrays
    it points into).  An ndarray needs unit stride along a row; its row stride is passed as the pitch."""
    ims = (DetectImage * max(len(images), 1))()
    keep = []
    for im, (ctx, img, staged) in zip(ims, images):
        im.ctx = ctx
        if img is not None:
            a = np.asarray(img)
            if a.dtype != np.uint8 or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 1) or a.strides[0] < a.shape[1]:
                a = np.ascontiguousarray(a, dtype=np.uint8)
            keep.append(a)
            im.image = a.ctypes.data_as(C.POINTER(C.c_uint8))
            im.height, im.width, im.pitch = a.shape[0], a.shape[1], a.strides[0]
        else:
            h, w = staged or (0, 0)
            im.height, im.width, im.pitch = h, w, w
    return ims, keep


def make_detect_params(rois, per_d, per_roi):
    """A DetectParams array: the defaults, then entry r's D (or None), ROI ((x, y, w, h) or None) and fields."""
    ps = (DetectParams * max(len(rois), 1))()
    for p, roi, d, kw in zip(ps, rois, per_d, per_roi):
        load().pfmpe_default_detect_params(C.byref(p))
        if d is not None:
            p.D[:] = list(np.asarray(d, np.float64).reshape(5))
        if roi is not None:
            p.roi_x, p.roi_y, p.roi_w, p.roi_h = [int(v) for v in roi]
        for k, v in (kw or {}).items():
            setattr(p, k, v)
    return ps


def _host_detect_batch(images, image_of, rois):
    """The C arrays of a host-only plan / pack call: images are ndarrays, or (h, w) shapes for staged images."""
    trip = [(None, None, tuple(im)) if isinstance(im, tuple) else (None, im, None) for im in images]
    ims, keep = make_detect_images(trip)
    R = len(rois)
    ps = make_detect_params(rois, [None] * R, [None] * R)
    idx = (C.c_int32 * max(R, 1))(*[int(i) for i in image_of])
    return ims, keep, ps, idx, R


def host_detect_plan(images, image_of, rois) -> tuple:
    """pfmpe_host_detect_plan: where the ROI pixels of a find_leds_streams batch land in its upload buffer.  images:
    ndarrays (host images), or (h, w) tuples for staged images; rois[r]: (x, y, w, h) or None in images[image_of[r]].
    Returns ([(offset, pitch, shared_with)] per entry, upload_bytes)."""
    ims, keep, ps, idx, R = _host_detect_batch(images, image_of, rois)
    crops = (DetectCrop * max(R, 1))()
    nbytes = C.c_int64()
    rc = load().pfmpe_host_detect_plan(ims, len(images), idx, ps, R, crops, C.byref(nbytes))
    if rc != OK:
        raise PFError(rc, "host_detect_plan: bad batch")
    return [(c.offset, c.pitch, c.shared_with) for c in crops[:R]], nbytes.value


def host_detect_pack(images, image_of, rois, crops=None, buffer_bytes=None) -> np.ndarray:
    """pfmpe_host_detect_pack: the upload buffer of a find_leds_streams batch (uint8): every own crop's rows at the
    planned offsets, every other byte 0.  crops / buffer_bytes default to the batch's plan."""
    ims, keep, ps, idx, R = _host_detect_batch(images, image_of, rois)
    if crops is None or buffer_bytes is None:
        plan, nbytes = host_detect_plan(images, image_of, rois)
        crops = plan if crops is None else crops
        buffer_bytes = nbytes if buffer_bytes is None else buffer_bytes
    cs = (DetectCrop * max(R, 1))(*[DetectCrop(*[int(v) for v in c]) for c in crops])
    buf = np.zeros(max(int(buffer_bytes), 1), dtype=np.uint8)
    rc = load().pfmpe_host_detect_pack(ims, len(images), idx, ps, R, cs, buf.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       int(buffer_bytes))
    if rc != OK:
        raise PFError(rc, "host_detect_pack: bad batch, crops that are not its plan, or a buffer too small")
    return buf[: int(buffer_bytes)]


def host_init_plan(M, B, num_cu: int) -> tuple:
    """pfmpe_host_init_plan: the work mapping of an initialise_multi batch's histogram stage.  M, B: markers and blobs
    per stream.  Returns (one dict per stream: items, first_block, blocks, bucket, lds_hist; blocks_per_bucket)."""
    m = np.ascontiguousarray(M, dtype=np.int32).reshape(-1)
    b = np.ascontiguousarray(B, dtype=np.int32).reshape(-1)
    if m.shape != b.shape:
        raise ValueError("host_init_plan: one M and one B per stream")
    S = int(m.shape[0])
    plan = (InitPlan * max(S, 1))()
    per_bucket = (C.c_int32 * 3)()
    i32 = C.POINTER(C.c_int32)
    rc = load().pfmpe_host_init_plan(m.ctypes.data_as(i32), b.ctypes.data_as(i32), S, int(num_cu), plan, per_bucket)
    if rc != OK:
        raise PFError(rc, "pfmpe_host_init_plan")
    return [plan[s].as_dict() for s in range(S)], list(per_bucket)


def host_cloud_plan(Ns) -> tuple:
    """pfmpe_host_cloud_plan: the grid of a cloud_stats_multi batch whose entries hold Ns[s] particles.  Returns (one
    dict per entry: first_block, blocks; the flat grid's size)."""
    n = np.ascontiguousarray(Ns, dtype=np.int32).reshape(-1)
    S = int(n.shape[0])
    plan = (CloudPlan * max(S, 1))()
    total = C.c_int32(0)
    rc = load().pfmpe_host_cloud_plan(n.ctypes.data_as(C.POINTER(C.c_int32)), S, plan, C.byref(total))
    if rc != OK:
        raise PFError(rc, "pfmpe_host_cloud_plan")
    return [plan[s].as_dict() for s in range(S)], int(total.value)


def host_refine_plan(K, B) -> tuple:
    """pfmpe_host_refine_plan: the packed upload buffer of a refine_multi batch.  K, B: hypotheses and blobs per stream.
    Returns (one dict per stream: first, model_offset, blobs_offset; the totals as a dict)."""
    k = np.ascontiguousarray(K, dtype=np.int32).reshape(-1)
    b = np.ascontiguousarray(B, dtype=np.int32).reshape(-1)
    if k.shape != b.shape:
        raise ValueError("host_refine_plan: one K and one B per stream")
    S = int(k.shape[0])
    plan = (RefinePlan * max(S, 1))()
    total = RefinePlanTotal()
    i32 = C.POINTER(C.c_int32)
    rc = load().pfmpe_host_refine_plan(k.ctypes.data_as(i32), b.ctypes.data_as(i32), S, plan, C.byref(total))
    if rc != OK:
        raise PFError(rc, "pfmpe_host_refine_plan")
    return [plan[s].as_dict() for s in range(S)], total.as_dict()


def host_grow_roi(roi, margin: int, image_w: int, image_h: int) -> tuple:
    """The reference's ROI enlargement (PE:429-432 / PE:454-457, pfmpe_host_grow_roi): (x, y, w, h) grown by
    `margin` on every side and clipped to the image as the reference clips it."""
    src = (C.c_int32 * 4)(*[int(v) for v in roi])
    dst = (C.c_int32 * 4)()
    rc = load().pfmpe_host_grow_roi(src, int(margin), int(image_w), int(image_h), dst)
    if rc != OK:
        raise PFError(rc, "host_grow_roi: margin < 0 or an image side < 1")
    return tuple(dst)


def host_philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    load().pfmpe_host_philox(c, k, o)
    return list(o)
