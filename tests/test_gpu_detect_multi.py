"""GPU parity of the batched LED detector (pfmpe_find_leds_multi) with the single-ROI call (pfmpe_find_leds) and
the CPU restatement (oracle/detect_oracle.cpp): every entry of a batch returns what its own single call returns,
same detections, same findContours order, identical float centres and double undistorted positions, the same
component count.  One 752 x 480 image of two objects whose tracking ROIs overlap; the single-call and oracle
results are computed once per (ROI, parameters) and shared."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

pytestmark = pytest.mark.gpu
K, D = syn.K_README, syn.D_README
W, H = 752, 480
ROI_A, ROI_B = (375, 187, 110, 127), (466, 245, 98, 109)
ROI_A20 = (355, 167, 150, 167)
CORNER = (707, 410, 45, 70)
T117 = {"threshold_value": 117}
SIGMA = {"gaussian_sigma": 1.3, "min_blob_area": 10.0, "max_blob_area": 400.0}
# the mixed batch of the parity test: (roi, parameters, detections the CPU oracle gives, or None)
MIXED = [
    (ROI_A, {}, 6), (ROI_B, {}, 5), (ROI_A20, {}, 9), (None, {}, 13), (None, T117, 609), (ROI_A20, T117, 50),
    (CORNER, T117, 5), ((0, 0, 33, 17), {}, 0), ((100, 100, 1, 1), {}, 0), ((300, 200, 2, 37), {}, 0),
    (ROI_A, SIGMA, None),
]
COMPONENTS = {(None, 117): 3442, (ROI_A20, 117): 251, (CORNER, 117): 38}


def pose_b():
    T = syn.truth_pose(0.5).copy()
    T[:3, 3] += np.array([0.55, 0.30, 0.6])
    return T


def make_engine(n=1000):
    eng = pf.Engine(device=0, max_particles=n)
    eng.set_model(syn.markers_for(5), K)
    return eng


class Scene:
    def __init__(self):
        ia, self.pa = syn.led_image(syn.truth_pose(0.5), syn.markers_for(5), seed=5, radius=4.5, noise=120)
        ib, self.pb = syn.led_image(pose_b(), syn.markers_for(5), seed=6, radius=3.2, noise=120, n_false=0)
        self.img = np.ascontiguousarray(np.maximum(ia, ib))
        self.inv = np.ascontiguousarray(255 - self.img)
        self.eng = make_engine()
        self._single, self._oracle = {}, {}

    @staticmethod
    def _key(roi, kw, inverted):
        return (roi, tuple(sorted(kw.items())), inverted)

    def single(self, roi, kw, inverted=False):
        """pfmpe_find_leds for this entry (once)."""
        k = self._key(roi, kw, inverted)
        if k not in self._single:
            self._single[k] = self.eng.find_leds(self.inv if inverted else self.img, D=D, roi=roi, **kw)
        return self._single[k]

    def oracle(self, roi, kw, inverted=False):
        k = self._key(roi, kw, inverted)
        if k not in self._oracle:
            okw = dict(kw)
            if "active_markers" in okw:
                okw["active_markers"] = bool(okw["active_markers"])
            self._oracle[k] = orc.find_leds(self.inv if inverted else self.img, K, D, roi=roi, **okw)[:2]
        return self._oracle[k]


@pytest.fixture(scope="module")
def sc():
    s = Scene()
    yield s
    s.eng.close()


def assert_entry(got, want, tag):
    (und, dist, info), (u1, d1, i1) = got, want
    assert info == i1, (tag, info, i1)
    assert info["overflow"] == 0, tag
    assert und.shape == u1.shape and dist.shape == d1.shape, (tag, und.shape, u1.shape)
    np.testing.assert_array_equal(und, u1, err_msg=str(tag))
    np.testing.assert_array_equal(dist, d1, err_msg=str(tag))


def check_batch(sc, entries, eng=None, staged=False, inverted=False):
    """One find_leds_multi over `entries` ((roi, kw) pairs), on the staged image if `staged`; every entry against
    its single call."""
    eng = eng or sc.eng
    img = None if staged else (sc.inv if inverted else sc.img)
    res = eng.find_leds_multi(img, rois=[e[0] for e in entries], D=D, params=[e[1] for e in entries])
    assert len(res) == len(entries)
    for r, (got, e) in enumerate(zip(res, entries)):
        assert_entry(got, sc.single(e[0], e[1], inverted), (r, e))
    return res


def test_scene_is_the_one_the_figures_are_for(sc):
    """The ROIs are the +-25 / +-20 px boxes around the two objects' ideal projections."""
    for ideal, roi in ((sc.pa, ROI_A), (sc.pb, ROI_B)):
        x0, y0 = int(ideal[:, 0].min()) - 25, int(ideal[:, 1].min()) - 20
        assert roi == (x0, y0, int(ideal[:, 0].max()) + 25 - x0, int(ideal[:, 1].max()) + 20 - y0)
    assert pf.host_grow_roi(ROI_A, 20, W, H) == ROI_A20


def test_parity_mixed_batch(sc):
    res = check_batch(sc, [(e[0], e[1]) for e in MIXED])
    for r, ((und, dist, info), (roi, kw, n_oracle)) in enumerate(zip(res, MIXED)):
        u_ref, d_ref = sc.oracle(roi, kw)
        np.testing.assert_array_equal(und, u_ref, err_msg=str(r))
        np.testing.assert_array_equal(dist, d_ref, err_msg=str(r))
        if n_oracle is not None:
            assert info["n"] == n_oracle, (r, info)
        nc = COMPONENTS.get((roi, kw.get("threshold_value")))
        if nc is not None:
            assert info["n_components"] == nc, (r, info)
    for r in (7, 8, 9):
        assert res[r][2]["n_components"] == 0


def test_order_and_isolation(sc):
    entries = [(e[0], e[1]) for e in MIXED]
    fwd = check_batch(sc, entries)
    rev = check_batch(sc, entries[::-1])
    for a, b in zip(fwd, rev[::-1]):
        assert_entry(a, b, "reversed")
    # an empty ROI between two busy ones
    check_batch(sc, [(ROI_A20, T117), ((100, 100, 1, 1), {}), (CORNER, T117)])


def test_giant_component(sc):
    """threshold 100 is below most of the 0..120 noise: one component covers the image and its merge crosses
    every tile border of the first entry."""
    t100 = {"threshold_value": 100}
    res = check_batch(sc, [(None, t100), (ROI_A, {})])
    assert res[0][2]["n"] == 0 and res[1][2]["n"] == 6
    assert res[0][2]["n_components"] == 1
    assert len(sc.oracle(None, t100)[0]) == 0


def grid64():
    return [(40 + 47 * (i % 8), 30 + 30 * (i // 8), 47, 30) for i in range(64)]


def test_r_limits(sc):
    assert_entry(sc.eng.find_leds_multi(sc.img, rois=[ROI_B], D=D)[0], sc.single(ROI_B, {}), "R = 1")
    res = check_batch(sc, [(roi, T117) for roi in grid64()])
    assert sum(info["n_components"] for _, _, info in res) > 64  # the grid is not empty
    with pytest.raises(pf.PFError) as ei:
        sc.eng.find_leds_multi(sc.img, rois=grid64() + [ROI_A], D=D)
    assert ei.value.code == pf.E_CAP


def raw_call(eng, img, entries, max_out, sentinel):
    """pfmpe_find_leds_multi on sentinel-filled arrays -> (rc, blobs, dist, outs)."""
    R = len(entries)
    ps = (pf.DetectParams * R)()
    for p, (roi, kw) in zip(ps, entries):
        eng.lib.pfmpe_default_detect_params(C.byref(p))
        p.D[:] = list(D)
        if roi is not None:
            p.roi_x, p.roi_y, p.roi_w, p.roi_h = roi
        for k, v in kw.items():
            setattr(p, k, v)
    blobs = np.full((R, max_out, 2), sentinel, dtype=np.float64)
    dist = np.full((R, max_out, 2), sentinel, dtype=np.float32)
    outs = (pf.DetectOut * R)()
    for o in outs:
        o.n = o.n_components = o.overflow = -77
    rc = eng.lib.pfmpe_find_leds_multi(eng.ctx, img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0],
                                       img.strides[0], ps, R, blobs.ctypes.data_as(C.POINTER(C.c_double)),
                                       dist.ctypes.data_as(C.POINTER(C.c_float)), max_out, outs)
    return rc, blobs, dist, outs


def test_truncation(sc):
    rc, blobs, dist, outs = raw_call(sc.eng, sc.img, [(ROI_A20, T117), (ROI_B, {})], 8, -5.0)
    assert rc == pf.OK
    u0, d0, i0 = sc.single(ROI_A20, T117)
    u1, d1, i1 = sc.single(ROI_B, {})
    assert outs[0].n == 50 == i0["n"] and outs[0].n_components == i0["n_components"]
    np.testing.assert_array_equal(blobs[0], u0[:8])
    np.testing.assert_array_equal(dist[0], d0[:8])
    assert outs[1].n == 5 == i1["n"]
    np.testing.assert_array_equal(blobs[1, :5], u1)
    np.testing.assert_array_equal(dist[1, :5], d1)
    assert np.all(blobs[1, 5:] == -5.0) and np.all(dist[1, 5:] == -5.0)


def test_buffer_reuse(sc):
    eng = make_engine()
    try:
        big = [(e[0], e[1]) for e in MIXED]
        check_batch(sc, big, eng=eng)
        check_batch(sc, [(CORNER, T117), (ROI_B, {})], eng=eng)
        assert_entry(eng.find_leds(sc.img, D=D, roi=ROI_A20, **T117), sc.single(ROI_A20, T117), "single between")
        check_batch(sc, big, eng=eng)
    finally:
        eng.close()


def test_passive_markers_per_entry(sc):
    check_batch(sc, [(None, {"active_markers": 0, "threshold_value": 14}), (None, {"active_markers": 1, **T117})],
                inverted=True)
    und, _, info = sc.single(None, {"active_markers": 0, "threshold_value": 14}, inverted=True)
    assert info["n"] > 0


def test_staged_image(sc):
    eng = make_engine()
    try:
        with pytest.raises(pf.PFError) as ei:
            eng.find_leds_multi(None, rois=[ROI_A, ROI_B], D=D)
        assert ei.value.code == pf.E_STATE
        eng.stage_image(sc.img)
        check_batch(sc, [(ROI_A, {}), (ROI_B, {}), (ROI_A20, T117)], eng=eng, staged=True)
    finally:
        eng.close()


def test_errors_launch_nothing(sc):
    good = [(ROI_A, {}), (ROI_B, {}), (ROI_A20, {}), (CORNER, T117)]
    bad_roi = good[:3] + [((700, 440, 53, 40), {})] + good[3:]  # entry 3 reaches one column past the image
    bad_sigma = [good[0], (ROI_B, {"gaussian_sigma": 0.0})] + good[2:]
    for entries, name in ((bad_roi, "roi 3"), (bad_sigma, "roi 1")):
        rc, blobs, dist, outs = raw_call(sc.eng, sc.img, entries, 16, -9.0)
        assert rc == pf.E_ARG
        msg = sc.eng.lib.pfmpe_last_error(sc.eng.ctx).decode()
        assert msg.startswith("find_leds_multi: " + name + ": "), msg
        assert np.all(blobs == -9.0) and np.all(dist == -9.0)
        assert all((o.n, o.n_components, o.overflow) == (-77, -77, -77) for o in outs)
        check_batch(sc, good)  # a correct call straight afterwards


def test_feeds_the_batched_step(sc):
    """Entries a and b of one batch drive one pfmpe_step_multi; two find_leds and two step calls give the same."""
    N = 4096
    poses = [syn.truth_pose(0.5), pose_b()]
    eye = np.eye(4)[:3].reshape(12)

    def engines():
        es = []
        for T in poses:
            e = make_engine(N)
            e.set_params(pf.default_params())
            e.set_prior(syn.initial_prior(T, N))
            es.append(e)
        return es

    solo, batch = engines(), engines()
    try:
        ref = []
        for e, T, roi in zip(solo, poses, (ROI_A, ROI_B)):
            blobs, _, _ = e.find_leds(sc.img, D=D, roi=roi)
            ref.append(e.step(e.make_frame(syn.to12(T), syn.to12(T), eye, blobs=blobs, seed=1)).as_dict())
        det = batch[0].find_leds_multi(sc.img, rois=[ROI_A, ROI_B], D=D)
        frames = [e.make_frame(syn.to12(T), syn.to12(T), eye, blobs=d[0], seed=1)
                  for e, T, d in zip(batch, poses, det)]
        outs = [o.as_dict() for o in pf.Engine.step_multi(batch, frames)]
        for s, (a, b) in enumerate(zip(outs, ref)):
            for k in a:
                if isinstance(a[k], np.ndarray):
                    assert np.array_equal(a[k], b[k], equal_nan=True), (s, k)
                else:
                    assert a[k] == b[k], (s, k, a[k], b[k])
            assert np.array_equal(batch[s].get_weights(), solo[s].get_weights()), s
        for s, b in enumerate(ref):
            assert b["accepted"] == 1 and b["n_corr"] == 5, (s, b["accepted"], b["n_corr"])
    finally:
        for e in solo + batch:
            e.close()


def test_timing_slot(sc):
    eng = make_engine()
    name = "k_det (detector pipeline)"
    try:
        eng.stage_image(sc.img)
        eng.find_leds(None, D=D, roi=ROI_A)
        eng.find_leds_multi(None, rois=[ROI_A, ROI_B], D=D)
        eng.set_option(pf.OPT_TIMING, 1)
        eng.reset_kernel_stats()
        eng.find_leds(None, D=D, roi=ROI_A)
        per_call, ms = eng.kernel_stats()[name]
        assert per_call >= 1 and ms > 0
        eng.reset_kernel_stats()
        eng.find_leds_multi(None, rois=[ROI_A, ROI_B, ROI_A20], D=D)
        n, ms = eng.kernel_stats()[name]
        assert n == per_call and ms > 0
        assert len(eng.kernel_stats()) == 9  # PFMPE_K_COUNT
    finally:
        eng.close()
