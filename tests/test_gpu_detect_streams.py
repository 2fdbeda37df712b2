"""GPU parity of the multi-camera LED detector (pfmpe_find_leds_streams) with the single-ROI call (pfmpe_find_leds)
on each camera's context and with the CPU restatement (oracle/detect_oracle.cpp): every entry of a batch returns
what its own single call returns, same detections, same findContours order, identical float centres and double
undistorted positions, the same component count.  Three cameras: 752 x 480 (K of the README), 96 x 64 with row
pitch 112 and another K, 33 x 17; the single-call and oracle results are computed once per entry and shared."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

pytestmark = pytest.mark.gpu
K0, D = syn.K_README, syn.D_README
K1 = K0.copy()
K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2] = K0[0, 0] * 1.1, K0[1, 1] * 0.9, K0[0, 2] - 20.0, K0[1, 2] + 15.0
D1 = np.array([-0.11, 0.03, 0.001, -0.002, 0.004])
D_ZERO = np.zeros(5)
W, H = 752, 480
ROI_A, ROI_B = (375, 187, 110, 127), (466, 245, 98, 109)
ROI_A20 = (355, 167, 150, 167)
CORNER = (707, 410, 45, 70)  # ends at the right and the bottom edge
T117 = {"threshold_value": 117}
SIGMA = {"gaussian_sigma": 1.3, "min_blob_area": 10.0, "max_blob_area": 400.0}
PASSIVE = {"active_markers": 0, "threshold_value": 14}
NAME = "k_det (detector pipeline)"
CAM0, CAM1, CAM2, CAM0_INV = 0, 1, 2, 3
# the mixed batch: (image, roi, parameters, D)
MIXED = [
    (CAM0, ROI_A, {}, D), (CAM0, ROI_A20, {}, D),          # the tracking ROI and its + 20 px retry: one crop
    (CAM2, None, {}, D), (CAM1, None, {}, D1),             # whole small images
    (CAM0, (100, 100, 1, 1), {}, D), (CAM0, (300, 200, 2, 37), {}, D),
    (CAM0, CORNER, T117, D), (CAM1, (50, 30, 46, 34), {}, D),  # ending at the right and bottom image edge
    (CAM0, ROI_A, SIGMA, D),                               # a second gaussian_sigma
    (CAM0_INV, ROI_A20, PASSIVE, D),                       # passive markers on the inverted image
    (CAM1, (10, 5, 60, 50), T117, D_ZERO), (CAM0, ROI_B, {}, D1),  # per-entry D
]


def pose_b():
    T = syn.truth_pose(0.5).copy()
    T[:3, 3] += np.array([0.55, 0.30, 0.6])
    return T


def make_engine(K=K0, n=1000, state=pf.STATE_F32):
    eng = pf.Engine(device=0, max_particles=n, state_dtype=state)
    eng.set_model(syn.markers_for(5), K)
    return eng


class Scene:
    def __init__(self):
        self.ia, self.pa = syn.led_image(syn.truth_pose(0.5), syn.markers_for(5), seed=5, radius=4.5, noise=120)
        self.ib, self.pb = syn.led_image(pose_b(), syn.markers_for(5), seed=6, radius=3.2, noise=120, n_false=0)
        img0 = np.ascontiguousarray(np.maximum(self.ia, self.ib))
        wide = np.full((64, 112), 255, dtype=np.uint8)  # the padding is bright: reading it would show
        wide[:, :96] = img0[200:264, 390:486]
        led = syn.distort_px(K0, D, self.pa)[0]
        x2, y2 = int(led[0]) - 16, int(led[1]) - 8
        self.imgs = [img0, wide[:, :96], np.ascontiguousarray(img0[y2:y2 + 17, x2:x2 + 33]),
                     np.ascontiguousarray(255 - img0)]
        self.Ks = [K0, K1, K0, K0]
        self.e0, self.e1, self.e2 = make_engine(K0), make_engine(K1, state=pf.STATE_F64), make_engine(K0, state=pf.STATE_F16)
        self.engs = [self.e0, self.e1, self.e2, self.e0]  # the leader appears under two images
        self._single, self._oracle = {}, {}

    def images(self):
        return list(zip(self.engs, self.imgs))

    @staticmethod
    def _key(e):
        cam, roi, kw, d = e
        return (cam, roi, tuple(sorted(kw.items())), tuple(d))

    def single(self, e):
        """pfmpe_find_leds on the entry's camera for this entry (once)."""
        k = self._key(e)
        if k not in self._single:
            cam, roi, kw, d = e
            self._single[k] = self.engs[cam].find_leds(self.imgs[cam], D=d, roi=roi, **kw)
        return self._single[k]

    def oracle(self, e):
        k = self._key(e)
        if k not in self._oracle:
            cam, roi, kw, d = e
            okw = dict(kw)
            if "active_markers" in okw:
                okw["active_markers"] = bool(okw["active_markers"])
            self._oracle[k] = orc.find_leds(self.imgs[cam], self.Ks[cam], d, roi=roi, **okw)[:2]
        return self._oracle[k]

    def close(self):
        for e in (self.e0, self.e1, self.e2):
            e.close()


@pytest.fixture(scope="module")
def sc():
    s = Scene()
    yield s
    s.close()


def assert_entry(got, want, tag):
    (und, dist, info), (u1, d1, i1) = got, want
    assert info == i1, (tag, info, i1)  # n, n_components, overflow
    assert info["overflow"] == 0, tag
    assert und.shape == u1.shape and dist.shape == d1.shape, (tag, und.shape, u1.shape)
    np.testing.assert_array_equal(und, u1, err_msg=str(tag))
    np.testing.assert_array_equal(dist, d1, err_msg=str(tag))


def run(images, entries):
    return pf.Engine.find_leds_streams(images, [e[0] for e in entries], [e[1] for e in entries],
                                       D=[e[3] for e in entries], params=[e[2] for e in entries])


def check_batch(sc, entries, images=None):
    res = run(images or sc.images(), entries)
    assert len(res) == len(entries)
    for r, (got, e) in enumerate(zip(res, entries)):
        assert_entry(got, sc.single(e), (r, e[:3]))
    return res


def test_the_plan_of_the_mixed_batch_shares_the_retry(sc):
    crops, nbytes = pf.host_detect_plan(sc.imgs, [e[0] for e in MIXED], [e[1] for e in MIXED])
    assert crops[0][2] == 1 and crops[8][2] == 1 and crops[7][2] == 3 and crops[10][2] == 3
    assert nbytes < W * H // 4


def test_parity_three_cameras(sc):
    res = check_batch(sc, MIXED)
    for r, ((und, dist, info), e) in enumerate(zip(res, MIXED)):
        u_ref, d_ref = sc.oracle(e)
        np.testing.assert_array_equal(und, u_ref, err_msg=str(r))
        np.testing.assert_array_equal(dist, d_ref, err_msg=str(r))
    n = [info["n"] for _, _, info in res]
    assert n[0] == 6 and n[1] == 9 and n[6] == 5 and n[4] == n[5] == 0  # the figures of the one-image batch's scene
    assert n[2] >= 1 and n[3] >= 1 and n[9] >= 1 and n[11] == 5, n      # every camera and the inverted image detect
    assert not np.array_equal(res[11][0], sc.single((CAM0, ROI_B, {}, D))[0])  # D is the entry's


def test_staged_and_host_mixed(sc):
    entries = [e for e in MIXED if e[0] in (CAM0, CAM1)]
    lead, never, other = make_engine(K0), make_engine(K0), make_engine(K0)
    try:
        lead.stage_image(sc.imgs[CAM0])
        images = [(lead, None), (sc.e1, sc.imgs[CAM1])]
        check_batch(sc, entries, images)
        # a context that never staged an image has none afterwards; one that staged X still detects on X
        other.stage_image(sc.imgs[CAM0_INV])
        e_inv = (CAM0_INV, ROI_A20, PASSIVE, D)
        res = run([(never, sc.imgs[CAM0]), (other, sc.imgs[CAM0]), (lead, None)],
                  [(0, ROI_A, {}, D), (1, ROI_A20, {}, D), (2, ROI_B, {}, D)])
        for got, e in zip(res, [(CAM0, ROI_A, {}, D), (CAM0, ROI_A20, {}, D), (CAM0, ROI_B, {}, D)]):
            assert_entry(got, sc.single(e), e[:3])
        p = pf.DetectParams()
        never.lib.pfmpe_default_detect_params(C.byref(p))
        blobs, out = np.zeros((8, 2)), pf.DetectOut()
        rc = never.lib.pfmpe_find_leds(never.ctx, None, W, H, W, C.byref(p), blobs.ctypes.data_as(C.POINTER(C.c_double)),
                                       None, 8, C.byref(out))
        assert rc == pf.E_STATE
        assert_entry(other.find_leds(None, D=D, roi=ROI_A20, **PASSIVE), sc.single(e_inv), "staged X")
        assert_entry(lead.find_leds(None, D=D, roi=ROI_A), sc.single((CAM0, ROI_A, {}, D)), "leader's staged image")
    finally:
        for e in (lead, never, other):
            e.close()


def test_64_entries_over_64_images(sc):
    yy, xx = np.mgrid[0:40, 0:40]
    imgs = []
    for i in range(64):
        cx, cy = 8.0 + (i % 8) * 3.4, 9.0 + (i // 8) * 3.1
        imgs.append(np.clip(np.rint(np.clip(5.0 - np.hypot(xx - cx, yy - cy), 0.0, 1.0) * 255.0 + (xx + i) % 7), 0,
                            255).astype(np.uint8))
    engs = [sc.e0 if i % 2 == 0 else sc.e1 for i in range(64)]
    want = [engs[i].find_leds(imgs[i], D=D) for i in range(64)]
    assert all(w[2]["n"] == 1 for w in want)
    assert not np.array_equal(want[0][0], sc.e1.find_leds(imgs[0], D=D)[0])  # K is the camera's
    images = list(zip(engs, imgs))
    fwd = pf.Engine.find_leds_streams(images, list(range(64)), [None] * 64, D=D)
    for i in range(64):
        assert_entry(fwd[i], want[i], i)
    rev = pf.Engine.find_leds_streams(images, list(range(63, -1, -1)), [None] * 64, D=D)
    for i in range(64):
        assert_entry(rev[i], want[63 - i], ("reversed", i))


def test_one_entry_and_reuse(sc):
    e = (CAM0, ROI_B, {}, D)
    assert_entry(run([(sc.e0, sc.imgs[CAM0])], [(0,) + e[1:]])[0], sc.single(e), "R = 1, I = 1")
    lead = make_engine(K0)
    try:
        images = [(lead, sc.imgs[0]), (sc.e1, sc.imgs[1]), (sc.e2, sc.imgs[2]), (lead, sc.imgs[3])]
        check_batch(sc, MIXED, images)
        check_batch(sc, [MIXED[7], MIXED[2]], images)  # a small batch after a larger one on the same leader
        check_batch(sc, MIXED, images)
    finally:
        lead.close()


def raw_call(images, n_images, image_of, entries, R, max_out, sentinel, null=()):
    """pfmpe_find_leds_streams on sentinel-filled arrays -> (rc, blobs, dist, outs).  images: (engine or None,
    array or None, staged (h, w) or None); null: names of the pointer arguments passed as NULL."""
    ims, keep = _capi.make_detect_images([(e.ctx if e is not None else None, img, st) for e, img, st in images])
    ps = _capi.make_detect_params([e[0] for e in entries], [e[2] for e in entries], [e[1] for e in entries])
    idx = (C.c_int32 * max(len(image_of), 1))(*image_of)
    n = max(len(entries), 1)
    blobs = np.full((n, max(max_out, 1), 2), sentinel, dtype=np.float64)
    dist = np.full((n, max(max_out, 1), 2), sentinel, dtype=np.float32)
    outs = (pf.DetectOut * n)()
    for o in outs:
        o.n = o.n_components = o.overflow = -77
    args = {"images": ims, "image_of": idx, "params": ps, "blobs": blobs.ctypes.data_as(C.POINTER(C.c_double)),
            "dist": dist.ctypes.data_as(C.POINTER(C.c_float)), "out": outs}
    for name in null:
        args[name] = None
    rc = pf.load().pfmpe_find_leds_streams(args["images"], n_images, args["image_of"], args["params"], R, args["blobs"],
                                           args["dist"], max_out, args["out"])
    return rc, blobs, dist, outs


def test_truncation(sc):
    entries = [(ROI_A20, T117, D), (ROI_A, {}, D), ((100, 100, 1, 1), {}, D)]
    rc, blobs, dist, outs = raw_call([(sc.e0, sc.imgs[0], None)], 1, [0, 0, 0], entries, 3, 2, -5.0)
    assert rc == pf.OK
    u0, d0, i0 = sc.single((CAM0, ROI_A20, T117, D))
    u1, d1, i1 = sc.single((CAM0, ROI_A, {}, D))
    assert outs[0].n == 50 == i0["n"] and outs[0].n_components == i0["n_components"]
    assert outs[1].n == 6 == i1["n"] and outs[2].n == 0
    np.testing.assert_array_equal(blobs[0], u0[:2])
    np.testing.assert_array_equal(dist[0], d0[:2])
    np.testing.assert_array_equal(blobs[1], u1[:2])
    np.testing.assert_array_equal(dist[1], d1[:2])
    assert np.all(blobs[2] == -5.0) and np.all(dist[2] == -5.0)
    # fewer detections than rows: the rows beyond them keep the sentinel
    rc, blobs, dist, outs = raw_call([(sc.e0, sc.imgs[0], None)], 1, [0, 0], entries[1:], 2, 8, -5.0)
    assert rc == pf.OK and outs[0].n == 6
    np.testing.assert_array_equal(blobs[0, :6], u1)
    assert np.all(blobs[0, 6:] == -5.0) and np.all(dist[0, 6:] == -5.0) and np.all(blobs[1] == -5.0)


def test_errors_launch_nothing(sc):
    lead, bare = make_engine(K0), pf.Engine(device=0, max_particles=1000)  # bare: no model
    try:
        lead.set_option(pf.OPT_TIMING, 1)
        lead.find_leds(sc.imgs[0], D=D, roi=ROI_A)
        lead.reset_kernel_stats()
        img0, img1 = sc.imgs[0], sc.imgs[1]
        one = [(lead, img0, None)]
        two = [(lead, img0, None), (sc.e1, img1, None)]
        good = [(ROI_A, {}, D), (ROI_B, {}, D)]
        grid = [((10 * (i % 8), 10 * (i // 8), 9, 9), {}, D) for i in range(65)]
        good2 = [(ROI_A, {}, D), ((10, 5, 60, 50), {}, D)]  # for the 96 x 64 camera as image 1
        cases = [  # name, images, I, image_of, entries, R, max_out, null pointers, code, error text starts with
            ("null image_of", one, 1, [0, 0], good, 2, 8, ("image_of",), pf.E_ARG, "find_leds_streams: "),
            ("null params", one, 1, [0, 0], good, 2, 8, ("params",), pf.E_ARG, "find_leds_streams: "),
            ("null out", one, 1, [0, 0], good, 2, 8, ("out",), pf.E_ARG, "find_leds_streams: "),
            ("null blobs", one, 1, [0, 0], good, 2, 8, ("blobs",), pf.E_ARG, "find_leds_streams: "),
            ("null ctx", [(lead, img0, None), (None, img1, None)], 2, [0, 1], good2, 2, 8, (), pf.E_ARG,
             "find_leds_streams: image 1: "),
            ("R < 1", one, 1, [0, 0], good, 0, 8, (), pf.E_ARG, "find_leds_streams: "),
            ("max_out < 0", one, 1, [0, 0], good, 2, -1, (), pf.E_ARG, "find_leds_streams: "),
            ("image index too large", two, 2, [0, 2], good, 2, 8, (), pf.E_ARG, "find_leds_streams: roi 1: "),
            ("image index negative", two, 2, [-1, 1], good, 2, 8, (), pf.E_ARG, "find_leds_streams: roi 0: "),
            ("roi outside", one, 1, [0, 0, 0], good + [((700, 440, 53, 40), {}, D)], 3, 8, (), pf.E_ARG,
             "find_leds_streams: roi 2: "),
            ("roi outside the smaller camera", two, 2, [0, 1], [good[0], ((50, 30, 47, 34), {}, D)], 2, 8, (), pf.E_ARG,
             "find_leds_streams: roi 1: "),
            ("sigma", one, 1, [0, 0], [(ROI_A, {"gaussian_sigma": 0.0}, D), good[1]], 2, 8, (), pf.E_ARG,
             "find_leds_streams: roi 0: "),
            ("R > 64", one, 1, [0] * 65, grid, 65, 8, (), pf.E_CAP, "find_leds_streams: "),
            ("I > 64", one * 65, 65, [0, 0], good, 2, 8, (), pf.E_CAP, "find_leds_streams: "),
            ("no model", [(lead, img0, None), (bare, img1, None)], 2, [0, 1], good2, 2, 8, (), pf.E_STATE,
             "find_leds_streams: image 1: "),
            ("nothing staged", [(lead, img0, None), (sc.e2, None, (H, W))], 2, [0, 1], good, 2, 8, (), pf.E_STATE,
             "find_leds_streams: image 1: "),
        ]
        for name, images, n_img, image_of, entries, R, max_out, null, code, text in cases:
            rc, blobs, dist, outs = raw_call(images, n_img, image_of, entries, R, max_out, -9.0, null)
            assert rc == code, name
            msg = lead.last_error()
            assert msg.startswith(text), (name, msg)
            assert np.all(blobs == -9.0) and np.all(dist == -9.0), name
            assert all((o.n, o.n_components, o.overflow) == (-77, -77, -77) for o in outs), name
        # an image of no width, a pitch below the width, a staged image of another pitch
        for field, value, code in (("width", 0, pf.E_ARG), ("height", 0, pf.E_ARG), ("pitch", W - 1, pf.E_ARG)):
            ims, keep = _capi.make_detect_images([(lead.ctx, img0, None)])
            ps = _capi.make_detect_params([ROI_A], [D], [{}])
            setattr(ims[0], field, value)
            out = pf.DetectOut(-77, -77, -77, 0)
            blobs = np.full((8, 2), -9.0)
            rc = lead.lib.pfmpe_find_leds_streams(ims, 1, (C.c_int32 * 1)(0), ps, 1,
                                                  blobs.ctypes.data_as(C.POINTER(C.c_double)), None, 8, C.byref(out))
            assert rc == code, field
            assert lead.last_error().startswith("find_leds_streams: image 0: "), lead.last_error()
            assert out.n == -77 and np.all(blobs == -9.0)
        lead.stage_image(img0)
        rc, _, _, outs = raw_call([(lead, None, (H, W - 1))], 1, [0], [((0, 0, 10, 10), {}, D)], 1, 8, -9.0)
        assert rc == pf.E_STATE and outs[0].n == -77
        # no leader: no text to fill
        rc, _, _, outs = raw_call(one, 1, [0, 0], good, 2, 8, -9.0, ("images",))
        assert rc == pf.E_ARG and outs[0].n == -77
        rc, _, _, outs = raw_call([(None, img0, None), (lead, img0, None)], 2, [0, 1], good, 2, 8, -9.0)
        assert rc == pf.E_ARG and outs[0].n == -77
        rc, _, _, outs = raw_call(one, 0, [0, 0], good, 2, 8, -9.0)
        assert rc == pf.E_ARG and outs[0].n == -77
        # (contexts on two devices are refused too: that takes a second device, which this suite does not assume)
        assert lead.kernel_stats()[NAME][0] == 0  # nothing was launched
        # a correct call straight afterwards
        res = run([(lead, None), (sc.e1, img1)], [(0, ROI_A, {}, D), (1, None, {}, D1)])
        assert_entry(res[0], sc.single((CAM0, ROI_A, {}, D)), "after the errors")
        assert_entry(res[1], sc.single((CAM1, None, {}, D1)), "after the errors")
        assert lead.kernel_stats()[NAME][0] > 0
    finally:
        lead.close()
        bare.close()


def test_timing_is_one_bracket_of_the_leader(sc):
    lead, member = make_engine(K0), make_engine(K1)
    try:
        images = [(lead, sc.imgs[0]), (member, sc.imgs[1])]
        entries = [(0, ROI_A, {}, D), (1, None, {}, D1), (0, ROI_A20, {}, D)]
        run(images, entries)
        lead.find_leds_multi(sc.imgs[0], rois=[ROI_A], D=D)
        for e in (lead, member):
            e.set_option(pf.OPT_TIMING, 1)
            e.reset_kernel_stats()
        lead.find_leds_multi(sc.imgs[0], rois=[ROI_A, ROI_B], D=D)
        per_bracket, ms = lead.kernel_stats()[NAME]
        assert per_bracket >= 1 and ms > 0
        lead.reset_kernel_stats()
        res = run(images, entries)
        n, ms = lead.kernel_stats()[NAME]
        assert n == per_bracket and ms > 0
        assert member.kernel_stats()[NAME] == (0, 0.0)
        assert all(v == (0, 0.0) for v in member.kernel_stats().values())
        assert len(lead.kernel_stats()) == 9  # PFMPE_K_COUNT
        assert_entry(res[1], sc.single((CAM1, None, {}, D1)), "timed batch")
        # the staged-only batch (no crop transfer) is one bracket too
        lead.stage_image(sc.imgs[0])
        lead.reset_kernel_stats()
        run([(lead, None)], [(0, ROI_A, {}, D)])
        assert lead.kernel_stats()[NAME][0] == per_bracket
    finally:
        lead.close()
        member.close()


def test_copy_command_variant_gives_the_same(sc):
    """The crop transfer as one async copy command (the A/B switch) instead of the pull kernel: the same results."""
    lead = make_engine(K0)
    try:
        lead.set_option(pf.OPT_DIAG, pf.DIAG_DET_COPY)
        images = [(lead, sc.imgs[0]), (sc.e1, sc.imgs[1]), (sc.e2, sc.imgs[2]), (lead, sc.imgs[3])]
        check_batch(sc, MIXED, images)
    finally:
        lead.close()


def test_feeds_the_batched_step(sc):
    """Two cameras, one object each: the detections of one batch drive one pfmpe_step_multi; two find_leds and two
    step calls give the same frame records.  N = 1000, fp64 state, the reference RNG."""
    N = 1000
    poses, imgs, rois = [syn.truth_pose(0.5), pose_b()], [sc.ia, sc.ib], [ROI_A, ROI_B]
    eye = np.eye(4)[:3].reshape(12)

    def engines():
        es = []
        for T in poses:
            e = make_engine(K0, N, pf.STATE_F64)
            prm = pf.default_params()
            prm.rng_mode = pf.RNG_REFERENCE
            e.set_params(prm)
            e.set_prior(syn.initial_prior(T, N))
            es.append(e)
        return es

    solo, batch = engines(), engines()
    try:
        ref = []
        for e, T, img, roi in zip(solo, poses, imgs, rois):
            blobs, _, _ = e.find_leds(img, D=D, roi=roi)
            assert len(blobs) >= 5
            ref.append(e.step(e.make_frame(syn.to12(T), syn.to12(T), eye, blobs=blobs, seed=1)).as_dict())
        det = pf.Engine.find_leds_streams(list(zip(batch, imgs)), [0, 1], rois, D=D)
        frames = [e.make_frame(syn.to12(T), syn.to12(T), eye, blobs=d[0], seed=1) for e, T, d in zip(batch, poses, det)]
        outs = [o.as_dict() for o in pf.Engine.step_multi(batch, frames)]
        for s, (a, b) in enumerate(zip(outs, ref)):
            for k in a:
                if isinstance(a[k], np.ndarray):
                    assert np.array_equal(a[k], b[k], equal_nan=True), (s, k)
                else:
                    assert a[k] == b[k], (s, k, a[k], b[k])
            assert np.array_equal(batch[s].get_weights(), solo[s].get_weights()), s
    finally:
        for e in solo + batch:
            e.close()
