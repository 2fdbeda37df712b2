"""Host side of the batched ROI prediction (pfmpe_predict_roi_multi, pfmpe_host_predict_roi): the binding's symbol
list, and pfmpe_host_predict_roi (the code a lane of the ROI kernels runs, then the host end every ROI entry point
shares) against the oracle's predictMarkerPositionsInImage + determineROI: the rectangle equal and the bits of bbox
equal, over cloud sizes, marker counts, camera motion, distortion, borders and image sizes; its edge cases; its
argument checks.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

EYE = np.eye(4)[:3].reshape(12)
D_ZERO = np.zeros(5)
T0 = syn.truth_pose(0.5)
_PRIORS = {}


def prior(N):
    if N not in _PRIORS:
        _PRIORS[N] = syn.initial_prior(T0, N, seed=40 + N)
    return _PRIORS[N]


def markers_of(M):
    if M <= 12:
        return syn.markers_for(M)
    rng = np.random.default_rng(16)  # no 16-LED model in the synthetic set: 12 known + random ones
    return np.vstack([syn.markers_12(), rng.uniform(-0.15, 0.3, size=(M - 12, 3))])


def cam_moved():
    cam = np.eye(4)
    cam[:3, :3] = syn.rot_z(0.01) @ syn.rot_x(-0.004)
    cam[:3, 3] = [0.01, -0.004, 0.002]
    return cam[:3].reshape(12)


def motion():
    """prediction matrix and predicted pose of a small constant-velocity step from T0"""
    Pm = syn.se3_exp(np.array([0.004, -0.002, 0.003, 0.002, -0.003, 0.004]))
    return syn.to12(Pm), syn.to12(T0 @ Pm)


def both(markers, K, D, poses, cam, prediction, predicted, w, h, border):
    got = pf.host_predict_roi(markers, K, poses,
                              pf.Engine.make_roi_in(prediction, predicted, D, w, h, border, cam_move_inv=cam))
    roi, bbox = orc.predict_roi(markers, K, D, np.asarray(poses, dtype=np.float64).reshape(-1, 12), cam, prediction,
                                predicted, w, h, border)
    return got, roi, bbox


def assert_same(got, roi, bbox, what):
    assert got["roi"] == roi, (what, got["roi"], roi)
    assert np.array_equal(got["bbox"].view(np.uint64), np.asarray(bbox).view(np.uint64)), (what, got["bbox"], bbox)


def test_symbols_are_listed_and_exported():
    lib = pf.load()
    for name in ("pfmpe_predict_roi_multi", "pfmpe_host_predict_roi"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert _capi.ROI_MAX_STREAMS == 64 and pf.ROI_MAX_STREAMS == 64
    # the batch strides: 3 x 12 + 5 doubles, 4 int32; 4 int32, 4 doubles
    assert C.sizeof(_capi.RoiIn) == 41 * 8 + 16 and C.sizeof(_capi.RoiOut) == 16 + 32


@pytest.mark.parametrize("M", [1, 5, 12, 16])
@pytest.mark.parametrize("N", [0, 1, 2, 300])
def test_host_predict_roi_equals_oracle(N, M):
    markers, K = markers_of(M), syn.K_README
    prediction, predicted = motion()
    poses = prior(N)
    seen = set()
    for cam, D, border, (w, h) in itertools.product((EYE, cam_moved()), (syn.D_README, D_ZERO), (0, 5, 20),
                                                    ((syn.IMAGE_W, syn.IMAGE_H), (64, 48))):
        got, roi, bbox = both(markers, K, D, poses, cam, prediction, predicted, w, h, border)
        assert_same(got, roi, bbox, (N, M, border, w, h))
        seen.add(tuple(roi))
    assert len(seen) > 1  # the sweep is not one constant answer (the small image alone gives another rectangle)


def test_make_roi_in_defaults_to_the_identity_camera_motion():
    ri = pf.Engine.make_roi_in(EYE, EYE, D_ZERO, 10, 20, 3)
    assert list(ri.cam_move_inv) == list(EYE) and (ri.image_w, ri.image_h, ri.border) == (10, 20, 3)


def test_pose_behind_the_camera_and_the_whole_image_fallback():
    """the "far" case of test_predict_roi_matches_oracle (the cloud behind the camera: mirrored projections), and a
    box narrower than one pixel (one LED, no particles, no border), which falls back to the whole image"""
    far = EYE.copy()
    far[11] = -5.0
    got, roi, bbox = both(syn.MARKERS_5, syn.K_README, syn.D_README, prior(300), far, EYE, far, syn.IMAGE_W,
                          syn.IMAGE_H, 10)
    assert_same(got, roi, bbox, "far")
    prediction, predicted = motion()
    got, roi, bbox = both(syn.MARKERS_5[:1], syn.K_README, syn.D_README, prior(0), EYE, prediction, predicted,
                          syn.IMAGE_W, syn.IMAGE_H, 0)
    assert_same(got, roi, bbox, "one point")
    assert roi == [0, 0, syn.IMAGE_W, syn.IMAGE_H] and bbox[0] == bbox[1] and bbox[2] == bbox[3]


def test_box_leaving_the_image_on_every_side_is_clamped():
    near = prior(300).copy()
    near[:, 3] = near[:, 3] * 0.1 - 0.14
    near[:, 7] *= 0.1
    near[:, 11] = 0.12  # the 0.2 .. 0.3 m marker frame 12 cm in front of the camera: projections far outside
    centre = syn.to12(syn.truth_pose(0.5))
    for D in (D_ZERO, syn.D_README):
        got, roi, bbox = both(syn.MARKERS_5, syn.K_README, D, near, EYE, EYE, centre, syn.IMAGE_W, syn.IMAGE_H, 5)
        assert_same(got, roi, bbox, "clamp")
    assert bbox[0] < 0 and bbox[1] > syn.IMAGE_W and bbox[2] < 0 and bbox[3] > syn.IMAGE_H
    assert roi == [0, 0, syn.IMAGE_W, syn.IMAGE_H]
    # one side each: a cloud shifted left / up keeps its right / lower edge
    left = prior(300).copy()  # the object's origin moved to project at pixel (10, 10)
    left[:, 3] += (10 - syn.K_README[0, 2]) / syn.K_README[0, 0] * T0[2, 3] - T0[0, 3]
    left[:, 7] += (10 - syn.K_README[1, 2]) / syn.K_README[1, 1] * T0[2, 3] - T0[1, 3]
    got, roi, bbox = both(syn.MARKERS_5, syn.K_README, D_ZERO, left, EYE, EYE, left[0], syn.IMAGE_W, syn.IMAGE_H, 5)
    assert_same(got, roi, bbox, "left")
    assert roi[0] == 0 and roi[1] == 0 and 0 < roi[2] < syn.IMAGE_W and 0 < roi[3] < syn.IMAGE_H


def test_nan_pose_never_wins():
    poses = prior(300).copy()
    prediction, predicted = motion()
    want = both(syn.MARKERS_5, syn.K_README, syn.D_README, np.delete(poses, 7, axis=0), EYE, prediction, predicted,
                syn.IMAGE_W, syn.IMAGE_H, 5)
    poses[7] = np.nan
    got, roi, bbox = both(syn.MARKERS_5, syn.K_README, syn.D_README, poses, EYE, prediction, predicted, syn.IMAGE_W,
                          syn.IMAGE_H, 5)
    assert_same(got, roi, bbox, "nan")
    assert np.all(np.isfinite(got["bbox"]))
    assert_same(got, want[1], want[2], "nan row = row left out")


def test_host_predict_roi_rejects_bad_arguments():
    lib = pf.load()
    dp = C.POINTER(C.c_double)
    m = np.ascontiguousarray(markers_of(16))
    k = np.ascontiguousarray(syn.K_README.reshape(9))
    p = np.ascontiguousarray(prior(2))
    mp, kp, pp = (a.ctypes.data_as(dp) for a in (m, k, p))
    ri = pf.Engine.make_roi_in(EYE, EYE, D_ZERO, 64, 48, 5)
    out = _capi.RoiOut(-7, -7, -7, -7, (C.c_double * 4)(-7.0, -7.0, -7.0, -7.0))
    call = lib.pfmpe_host_predict_roi
    assert call(None, 5, kp, pp, 2, C.byref(ri), C.byref(out)) == pf.E_ARG
    assert call(mp, 5, None, pp, 2, C.byref(ri), C.byref(out)) == pf.E_ARG
    assert call(mp, 5, kp, None, 2, C.byref(ri), C.byref(out)) == pf.E_ARG
    assert call(mp, 5, kp, pp, 2, None, C.byref(out)) == pf.E_ARG
    assert call(mp, 5, kp, pp, 2, C.byref(ri), None) == pf.E_ARG
    assert call(mp, 0, kp, pp, 2, C.byref(ri), C.byref(out)) == pf.E_ARG
    assert call(mp, pf.MAX_MARKERS + 1, kp, pp, 2, C.byref(ri), C.byref(out)) == pf.E_ARG
    assert call(mp, 5, kp, pp, -1, C.byref(ri), C.byref(out)) == pf.E_ARG
    for w, h in ((0, 48), (64, 0), (-3, 48)):
        bad = pf.Engine.make_roi_in(EYE, EYE, D_ZERO, w, h, 5)
        assert call(mp, 5, kp, pp, 2, C.byref(bad), C.byref(out)) == pf.E_ARG
    assert [out.x, out.y, out.width, out.height] + list(out.bbox) == [-7] * 8
    assert call(mp, 5, kp, None, 0, C.byref(ri), C.byref(out)) == pf.OK  # poses may be NULL when N = 0
    assert call(mp, pf.MAX_MARKERS, kp, pp, 2, C.byref(ri), C.byref(out)) == pf.OK
    with pytest.raises(pf.PFError):
        pf.host_predict_roi(m[:5], k, p, pf.Engine.make_roi_in(EYE, EYE, D_ZERO, 0, 48, 5))
