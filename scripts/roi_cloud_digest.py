"""Digests of the single ROI and cloud-statistics calls, one sha256 per case over the raw pfmpe_roi_out /
pfmpe_cloud_out bytes, for comparing two builds of the library bit for bit (run it on each build and diff the two
outputs; profiles/single_as_batch/ holds such a pair).

Cases, all with the Philox generator: the three state types at N = 1, 63, 64, 257, 1000, 4097 and 65,537 (257 blocks:
the ROI's final block makes a second pass over the partials), and fp32 / fp16 at N = 300,001 with two-launch frames
(1,172 particle blocks on the cloud's 1,024-block grid; the prior is deferred and read through owner indices).  Per
case: pfmpe_cloud_stats(POSTERIOR) of the bare prior about its first particle, pfmpe_predict_roi with an identity and
a non-identity cam_move_inv; then, after two steps, WEIGHTED and POSTERIOR about the last step's pose and the two ROIs
of the next frame.
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import _capi  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402

STATES = (("f64", pf.STATE_F64), ("f32", pf.STATE_F32), ("f16", pf.STATE_F16))
SIZES = (1, 63, 64, 257, 1000, 4097, 65_537)
LARGE = 300_001
DP = C.POINTER(C.c_double)


def cam_moved():
    cam = np.eye(4)
    cam[:3, :3] = syn.rot_z(0.004) @ syn.rot_x(-0.003)
    cam[:3, 3] = [0.01, -0.008, 0.002]
    return cam[:3].reshape(12)


def sha(raw):
    return hashlib.sha256(raw).hexdigest()


def cloud(eng, which, ref):
    out = _capi.CloudOut()
    r = np.ascontiguousarray(ref, dtype=np.float64)
    if eng.lib.pfmpe_cloud_stats(eng.ctx, which, r.ctypes.data_as(DP), C.byref(out)) != pf.OK:
        raise RuntimeError(eng.last_error())
    return sha(bytes(out))


def roi(eng, fr, cam):
    rin = pf.Engine.make_roi_in(fr.prediction, fr.predicted_pose, syn.D_README, syn.IMAGE_W, syn.IMAGE_H, 5,
                                cam_move_inv=cam)
    out = _capi.RoiOut()
    if eng.lib.pfmpe_predict_roi(eng.ctx, C.byref(rin), C.byref(out)) != pf.OK:
        raise RuntimeError(eng.last_error())
    return sha(bytes(out))


def case(st, sname, state, N, fused):
    eng = pf.Engine(device=0, max_particles=N, state_dtype=state)
    try:
        eng.set_option(pf.OPT_FUSED, fused)
        eng.set_model(st.markers, st.K)
        prm = pf.default_params()
        prm.rng_mode = pf.RNG_PHILOX
        eng.set_params(prm)
        prior = syn.initial_prior_fast(syn.to44(st.frames[0].current_pose), N, seed=7)
        eng.set_prior(prior)
        name = f"{sname}_N{N}"
        print(f"{name} prior cloud_posterior {cloud(eng, pf.CLOUD_POSTERIOR, prior[0].reshape(12))}")
        print(f"{name} prior roi_identity {roi(eng, st.frames[0], None)}")
        print(f"{name} prior roi_cam_moved {roi(eng, st.frames[0], cam_moved())}")
        for f in (0, 1):
            fr = st.frames[f]
            out = eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                          seed=900 + f, frame_idx=f))
        if N == LARGE and eng.info(pf.INFO_LAST_RESAMPLE) != pf.RESAMPLE_OWNERS:
            raise RuntimeError("the large case's prior is not deferred")
        ref = np.array(out.winner_pose if out.resampled else out.most_likely_pose)
        print(f"{name} stepped cloud_weighted {cloud(eng, pf.CLOUD_WEIGHTED, ref)}")
        print(f"{name} stepped cloud_posterior {cloud(eng, pf.CLOUD_POSTERIOR, ref)}")
        print(f"{name} stepped roi_identity {roi(eng, st.frames[2], None)}")
        print(f"{name} stepped roi_cam_moved {roi(eng, st.frames[2], cam_moved())}", flush=True)
    finally:
        eng.close()


def main():
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=50, N=1000), 3)
    for sname, state in STATES:
        for N in SIZES:
            case(st, sname, state, N, 2)
    for sname, state in STATES[1:]:
        case(st, sname, state, LARGE, 0)


if __name__ == "__main__":
    main()
