"""The timing brackets of the host-synchronous timed entries (detector, ROI prediction, initialisation).

Per call, with PFMPE_OPT_TIMING off and on:
  1. timing off: kernel_stats() is unchanged by the call;
  2. timing on: the kernel ids whose launch count moves are the call's own (the detector id for the detector calls,
     the ROI id for the ROI calls, for the initialisation whatever its first call shows), a second identical call
     moves them by the same amounts, and total_ms grows for exactly those ids;
  3. after an argument error with timing on (gaussian_sigma = 0; image_w = 0 for the ROI) the next good call shows the
     increments of 2;
  4. two consecutive kernel_stats() reads at the end are equal: nothing is left pending.
The paths on which a launch fails inside a timed entry are not reachable from a test."""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi
from pf_monocular_pose_estimator_amd import synthetic as syn

pytestmark = pytest.mark.gpu

N, M = 300, 5
DET, ROI = "k_det (detector pipeline)", "k_roi"
DET_PRM = {"min_blob_area": 5.0}
BAD_PRM = {"min_blob_area": 5.0, "gaussian_sigma": 0.0}
ROIS = [None, (4, 4, 40, 30)]


class Rig:
    """Two fp32 engines with a prior each; the first has the image staged and makes every call."""

    def __init__(self):
        self.st = syn.make_stream(syn.StreamConfig("t", M=M, B=20, N=N), 1)
        self.fr = self.st.frames[0]
        self.engines = []
        for i in range(2):
            eng = pf.Engine(device=0, max_particles=N, state_dtype=pf.STATE_F32)
            eng.set_model(self.st.markers, self.st.K)
            eng.set_params(pf.default_params())
            eng.set_prior(syn.initial_prior_fast(syn.to44(self.fr.current_pose), N, seed=7 + i))
            self.engines.append(eng)
        self.a = self.engines[0]
        self.img = np.zeros((48, 64), np.uint8)
        self.img[8:13, 10:15] = 255
        self.img[30:35, 40:45] = 255
        self.a.stage_image(self.img)
        self.blobs, _ = syn.init_blobs(M, 3, seed=0)

    def roi_in(self, image_w=752):
        return pf.Engine.make_roi_in(self.fr.prediction, self.fr.predicted_pose, syn.D_README, image_w, 480, 5)

    def calls(self):
        """name -> (the call, the same with an argument error or None, its kernel ids or None)"""
        a, fr = self.a, self.fr

        def roi(image_w):
            return a.predict_roi(fr.prediction, fr.predicted_pose, syn.D_README, image_w, 480, 5)

        return {
            "find_leds_staged": (lambda: a.find_leds(**DET_PRM), lambda: a.find_leds(**BAD_PRM), {DET}),
            "find_leds_host": (lambda: a.find_leds(self.img, **DET_PRM), lambda: a.find_leds(self.img, **BAD_PRM), {DET}),
            "find_leds_multi": (lambda: a.find_leds_multi(rois=ROIS, params=DET_PRM),
                                lambda: a.find_leds_multi(rois=ROIS, params=BAD_PRM), {DET}),
            "find_leds_streams": (lambda: pf.Engine.find_leds_streams([(a, None)], [0], [None], params=DET_PRM),
                                  lambda: pf.Engine.find_leds_streams([(a, None)], [0], [None], params=BAD_PRM), {DET}),
            "predict_roi": (lambda: roi(752), lambda: roi(0), {ROI}),
            "predict_roi_multi": (lambda: pf.Engine.predict_roi_multi(self.engines, [self.roi_in()] * 2),
                                  lambda: pf.Engine.predict_roi_multi(self.engines, [self.roi_in(), self.roi_in(0)]),
                                  {ROI}),
            "p3p_histogram": (lambda: a.p3p_histogram(self.blobs), None, None),
            "initialise": (lambda: a.initialise(self.blobs, n_particles=N), None, None),
        }


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    for e in r.engines:
        e.close()


def moved(before, after):
    """(launch-count increments of the ids that moved, the ids whose total_ms grew)"""
    counts = {k: after[k][0] - before[k][0] for k in after if after[k][0] != before[k][0]}
    grew = {k for k in after if after[k][1] > before[k][1]}
    assert all(after[k][1] >= before[k][1] for k in after)
    return counts, grew


CALLS = ["find_leds_staged", "find_leds_host", "find_leds_multi", "find_leds_streams", "predict_roi",
         "predict_roi_multi", "p3p_histogram", "initialise"]


@pytest.mark.parametrize("name", CALLS)
def test_brackets_of_call(rig, name):
    good, bad, own = rig.calls()[name]
    a = rig.a
    a.set_option(pf.OPT_TIMING, 0)
    s0 = a.kernel_stats()
    res = good()
    assert a.kernel_stats() == s0, "timing off: the call moved the statistics"
    if name == "find_leds_staged":
        assert res[2]["n_components"] == 2  # the image is what the docstring says
    a.set_option(pf.OPT_TIMING, 1)
    try:
        s0 = a.kernel_stats()
        good()
        s1 = a.kernel_stats()
        good()
        s2 = a.kernel_stats()
        first, grew1 = moved(s0, s1)
        second, grew2 = moved(s1, s2)
        print(name, "increments", first, "ms", {k: s1[k][1] - s0[k][1] for k in first})
        assert first and all(v > 0 for v in first.values())
        if own is not None:
            assert set(first) == own
        assert second == first
        assert grew1 == set(first) and grew2 == set(first)
        if bad is not None:
            with pytest.raises(pf.PFError) as err:
                bad()
            assert err.value.code == _capi.E_ARG
            s3 = a.kernel_stats()
            assert s3 == s2, "an argument error moved the statistics"
            good()
            third, grew3 = moved(s3, a.kernel_stats())
            assert third == first and grew3 == set(first)
        assert a.kernel_stats() == a.kernel_stats(), "a bracket was left pending"
    finally:
        a.set_option(pf.OPT_TIMING, 0)
