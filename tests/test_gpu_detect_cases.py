"""The LED detector on the device over the case suite of tests/detect_cases.py (checked without a GPU by
tests/test_detect_cases_host.py): shapes, ROI sizes and caps the scene tests never meet.

The bar is the detector's own: the pipeline is integer up to a same-order double tail, so pfmpe_find_leds equals the
oracle bit for bit (same detections, same order, same float centres, same double undistorted positions), and every
entry of a pfmpe_find_leds_multi / pfmpe_find_leds_streams batch equals its single call byte for byte.  The device's
n_components is held to the flood-fill count of the numpy mask, which ties the mask, labelling, merge and roots kernels
to something that is not the oracle.  One engine serves the module; a single call's result is computed once."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

import detect_cases as dc

pytestmark = pytest.mark.gpu
K, D = dc.K, dc.D
K1 = K.copy()
K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2] = K[0, 0] * 1.1, K[1, 1] * 0.9, K[0, 2] - 20.0, K[1, 2] + 15.0
PLAIN = dc.names("zoo") + dc.names("translate") + dc.names("sweep")   # every case below the caps
BATCHES = dc.batches(PLAIN)
U8P = C.POINTER(C.c_uint8)


def make_engine(k=K, state=pf.STATE_F32):
    eng = pf.Engine(device=0, max_particles=1000, state_dtype=state)
    eng.set_model(syn.markers_for(5), k)
    return eng


class Scene:
    def __init__(self):
        self.eng = make_engine()
        self._single = {}

    def single(self, name):
        """pfmpe_find_leds on the case (once)."""
        if name not in self._single:
            c = dc.case(name)
            self._single[name] = self.eng.find_leds(c.image, D=D, roi=c.roi, **c.prm)
        return self._single[name]


@pytest.fixture(scope="module")
def sc():
    s = Scene()
    yield s
    s.eng.close()


def assert_bytes(got, want, tag):
    """A batch entry against its single call: the same bytes."""
    (und, dist, info), (u1, d1, i1) = got, want
    assert info == i1, (tag, info, i1)
    assert und.shape == u1.shape and dist.shape == d1.shape, (tag, und.shape, u1.shape)
    assert und.tobytes() == u1.tobytes() and dist.tobytes() == d1.tobytes(), tag


def assert_oracle(got, name, tag=None):
    und, dist, info = got
    u_ref, d_ref, _, _, stats = dc.oracle(name)
    assert info["n"] == stats["n"] and info["overflow"] == 0, (tag or name, info, stats)
    assert dc.same_bits(und, u_ref) and dc.same_bits(dist, d_ref), tag or name


def fill_params(eng, ps, cases):
    for p, c in zip(ps, cases):
        eng.lib.pfmpe_default_detect_params(C.byref(p))
        p.D[:] = list(D)
        if c.roi is not None:
            p.roi_x, p.roi_y, p.roi_w, p.roi_h = c.roi
        for k, v in c.prm.items():
            setattr(p, k, v)


def raw_single(eng, img, c, max_out=dc.MAX_BLOBS, sentinel=-5.0):
    """pfmpe_find_leds on `img` as it lies in memory (any row pitch), sentinel-filled arrays -> (blobs, dist, out)."""
    ps = (pf.DetectParams * 1)()
    fill_params(eng, ps, [c])
    blobs = np.full((max(max_out, 1), 2), sentinel, dtype=np.float64)
    dist = np.full((max(max_out, 1), 2), sentinel, dtype=np.float32)
    out = pf.DetectOut()
    rc = eng.lib.pfmpe_find_leds(eng.ctx, img.ctypes.data_as(U8P), img.shape[1], img.shape[0], img.strides[0], ps,
                                 blobs.ctypes.data_as(C.POINTER(C.c_double)), dist.ctypes.data_as(C.POINTER(C.c_float)),
                                 max_out, C.byref(out))
    assert rc == pf.OK, eng.lib.pfmpe_last_error(eng.ctx).decode()
    return blobs, dist, out


def raw_multi(eng, img, cases, max_out=dc.MAX_BLOBS, sentinel=-5.0):
    """pfmpe_find_leds_multi likewise -> (blobs R x max_out x 2, dist, outs)."""
    R = len(cases)
    ps = (pf.DetectParams * R)()
    fill_params(eng, ps, cases)
    blobs = np.full((R, max(max_out, 1), 2), sentinel, dtype=np.float64)
    dist = np.full((R, max(max_out, 1), 2), sentinel, dtype=np.float32)
    outs = (pf.DetectOut * R)()
    rc = eng.lib.pfmpe_find_leds_multi(eng.ctx, img.ctypes.data_as(U8P), img.shape[1], img.shape[0], img.strides[0], ps,
                                       R, blobs.ctypes.data_as(C.POINTER(C.c_double)),
                                       dist.ctypes.data_as(C.POINTER(C.c_float)), max_out, outs)
    assert rc == pf.OK, eng.lib.pfmpe_last_error(eng.ctx).decode()
    return blobs, dist, outs


def assert_raw(blobs, dist, out, want, tag, sentinel=-5.0):
    """The rows and the record of a raw call against a single call's result; nothing behind the rows is touched."""
    u1, d1, i1 = want
    assert (out.n, out.n_components, out.overflow) == (i1["n"], i1["n_components"], i1["overflow"]), tag
    n = len(u1)
    assert blobs[:n].tobytes() == u1.tobytes() and dist[:n].tobytes() == d1.tobytes(), tag
    assert np.all(blobs[n:] == sentinel) and np.all(dist[n:] == sentinel), tag


# ---------------------------------------------------------------------------------------- the single call
@pytest.mark.parametrize("name", PLAIN)
def test_single_call_matches_oracle_and_yardstick(sc, name):
    got = sc.single(name)
    assert_oracle(got, name)
    assert got[2]["n_components"] == dc.yardstick(name)[1], (name, got[2])


# ---------------------------------------------------------------------------------------- batches of one image
@pytest.mark.parametrize("b", range(len(BATCHES)))
def test_multi_batch_equals_single_calls(sc, b):
    names = BATCHES[b]
    if b % 3 == 1:
        names = names[::-1]
    cs = [dc.case(n) for n in names]
    res = sc.eng.find_leds_multi(cs[0].image, rois=[c.roi for c in cs], D=D, params=[c.prm for c in cs])
    assert len(res) == len(cs)
    for r, (got, n) in enumerate(zip(res, names)):
        assert_bytes(got, sc.single(n), (b, r, n))
        assert_oracle(got, n, (b, r, n))


def test_multi_batch_reversed(sc):
    """The largest batch forwards and backwards: an entry's result does not depend on its place."""
    names = max(BATCHES, key=len)
    assert len(names) == 64
    cs = [dc.case(n) for n in names]
    fwd = sc.eng.find_leds_multi(cs[0].image, rois=[c.roi for c in cs], D=D, params=[c.prm for c in cs])
    rev = sc.eng.find_leds_multi(cs[0].image, rois=[c.roi for c in cs[::-1]], D=D, params=[c.prm for c in cs[::-1]])
    for r, (a, z, n) in enumerate(zip(fwd, rev[::-1], names)):
        assert_bytes(a, z, (r, n))
        assert_bytes(a, sc.single(n), (r, n))


# ---------------------------------------------------------------------------------------- row pitch above the width
@pytest.mark.parametrize("extra", [1, 37])
def test_padded_pitch_single(sc, extra):
    """Every case through pfmpe_find_leds with the image in a buffer of pitch width + extra, the padding at 255."""
    views = {}
    for n in PLAIN:
        c = dc.case(n)
        if c.image_id not in views:
            views[c.image_id] = dc.padded(c.image, extra)
        img = views[c.image_id]
        assert img.strides[0] == c.image.shape[1] + extra
        blobs, dist, out = raw_single(sc.eng, img, c)
        assert_raw(blobs, dist, out, sc.single(n), (extra, n))


@pytest.mark.parametrize("extra", [1, 37])
def test_padded_pitch_multi(sc, extra):
    for b, names in enumerate(BATCHES):
        cs = [dc.case(n) for n in names]
        img = dc.padded(cs[0].image, extra)
        blobs, dist, outs = raw_multi(sc.eng, img, cs)
        for r, n in enumerate(names):
            assert_raw(blobs[r], dist[r], outs[r], sc.single(n), (extra, b, r, n))


# ---------------------------------------------------------------------------------------- several cameras
def streams_batch():
    """The entries of the two-camera batch: the cases of the first zoo image (camera 0) and of the second (camera 1),
    interleaved, plus the enlargement (pfmpe_host_grow_roi, 20 px) of the smallest ROI of camera 0."""
    zoo = dc.cases("zoo")
    ids = sorted({c.image_id for c in zoo})
    on0 = [c for c in zoo if c.image_id == ids[0]]
    on1 = [c for c in zoo if c.image_id == ids[1]]
    img0, img1 = on0[0].image, on1[0].image
    base = min(on0, key=lambda c: c.rect[2] * c.rect[3])
    grown = dc.Case("grown", "zoo", base.image_id, img0,
                    pf.host_grow_roi(base.roi, 20, img0.shape[1], img0.shape[0]), base.prm)
    entries = [(0, c) for c in on0] + [(0, grown)] + [(1, c) for c in on1]
    entries = entries[::2] + entries[1::2]
    return img0, img1, entries, base, grown


def test_streams_two_contexts(sc):
    """One pfmpe_find_leds_streams batch over two contexts with different K: the first zoo image from host memory with a
    padded pitch (only its ROIs' pixels are uploaded; an ROI and its enlargement share one crop), the second staged
    on its context."""
    img0, img1, entries, base, grown = streams_batch()
    image_of = [e[0] for e in entries]
    cs = [e[1] for e in entries]
    crops, _ = pf.host_detect_plan([dc.padded(img0, 37), img1.shape], image_of, [c.roi for c in cs])
    assert crops[cs.index(base)][2] == cs.index(grown)   # the shared crop
    e1 = make_engine(K1, state=pf.STATE_F64)
    try:
        e1.stage_image(img1)
        res = pf.Engine.find_leds_streams([(sc.eng, dc.padded(img0, 37)), (e1, None)], image_of, [c.roi for c in cs],
                                          D=D, params=[c.prm for c in cs])
        assert len(res) == len(cs)
        for r, (got, (cam, c)) in enumerate(zip(res, entries)):
            eng, k, img = (sc.eng, K, img0) if cam == 0 else (e1, K1, img1)
            assert_bytes(got, eng.find_leds(img, D=D, roi=c.roi, **c.prm), (r, c.name))
            u_ref, d_ref, _, _ = orc.find_leds(img, k, D, roi=c.roi, **c.prm)
            assert dc.same_bits(got[0], u_ref) and dc.same_bits(got[1], d_ref), (r, c.name)
            assert got[2]["overflow"] == 0
        assert res[cs.index(grown)][2]["n"] >= res[cs.index(base)][2]["n"] >= 1
    finally:
        e1.close()


# ---------------------------------------------------------------------------------------- the caps
def test_cap_a_all_8192_slots(sc):
    got = sc.single("cap_a_8192")
    assert got[2] == {"n": 0, "n_components": 8192, "overflow": 0}
    assert dc.yardstick("cap_a_8192")[1] == 8192
    assert_oracle(got, "cap_a_8192")


def test_cap_b_overflow(sc):
    got = sc.single("cap_b_8256")
    assert got[2] == {"n": 0, "n_components": 8256, "overflow": 1}
    assert dc.yardstick("cap_b_8256")[1] == 8256 and len(got[0]) == 0


def test_cap_c_overflow_returns_a_subsequence(sc):
    """8261 components, 8192 slots handed out in atomic order: which components are examined is not fixed, but what
    is returned are rows of the oracle's list, in its order."""
    name = "cap_c_8256_discs"
    und, dist, info = sc.single(name)
    assert info["overflow"] == 1 and info["n_components"] == dc.yardstick(name)[1] == 8261
    u_ref, d_ref, _, _, stats = dc.oracle(name, 100000)
    assert stats["n"] == len(u_ref) == 5 and info["n"] == len(und) <= 5
    at = 0
    for u, d in zip(und, dist):
        while at < len(u_ref) and not (u.tobytes() == u_ref[at].tobytes() and d.tobytes() == d_ref[at].tobytes()):
            at += 1
        assert at < len(u_ref), (und, u_ref)
        at += 1


def test_cap_d_more_detections_than_rows(sc):
    name = "cap_d_1225"
    c = dc.case(name)
    u_ref, d_ref, _, _, stats = dc.oracle(name, 2000)
    assert stats["n"] == len(u_ref) == 1225
    for max_out in (2000, 0, 1, 1023):
        blobs, dist, out = raw_single(sc.eng, c.image, c, max_out=max_out, sentinel=-7.0)
        assert (out.n, out.n_components, out.overflow) == (1225, 1225, 0), max_out
        n = min(max_out, dc.MAX_BLOBS)
        assert dc.same_bits(blobs[:n], u_ref[:n]) and dc.same_bits(dist[:n], d_ref[:n]), max_out
        assert np.all(blobs[n:] == -7.0) and np.all(dist[n:] == -7.0), max_out
    # the Python layer returns the rows that were written, whatever max_out
    und, dist, info = sc.eng.find_leds(c.image, D=D, max_out=2000, **c.prm)
    assert info["n"] == 1225 and und.shape == (1024, 2) and dist.shape == (1024, 2)
    assert dc.same_bits(und, u_ref[:1024]) and dc.same_bits(dist, d_ref[:1024])
    (um, dm, im), = sc.eng.find_leds_multi(c.image, rois=[None], D=D, params=[c.prm], max_out=2000)
    assert im == info and um.tobytes() == und.tobytes() and dm.tobytes() == dist.tobytes()
    (us, ds, is_), = pf.Engine.find_leds_streams([(sc.eng, c.image)], [0], [None], D=D, params=[c.prm], max_out=2000)
    assert is_ == info and us.tobytes() == und.tobytes() and ds.tobytes() == dist.tobytes()


def test_caps_inside_a_batch(sc):
    """The overflowing lattice and the 1225-detection lattice as entries of a batch beside an ordinary ROI: that ROI's
    result is its single call's, and the capped entries are theirs."""
    c = dc.case("cap_c_8256_discs")
    lattice = dc.Case("lattice", "cap", c.image_id, c.image, (0, 0, 259, 129), {"threshold_value": 1})
    discs = dc.Case("discs", "cap", c.image_id, c.image, (3, 131, 253, 19), {"min_blob_area": 0.0})
    cs = [discs, lattice, discs]
    res = sc.eng.find_leds_multi(c.image, rois=[e.roi for e in cs], D=D, params=[e.prm for e in cs])
    want = sc.eng.find_leds(c.image, D=D, roi=discs.roi, **discs.prm)
    assert want[2] == {"n": 5, "n_components": 5, "overflow": 0}
    u_ref, d_ref, _, _ = orc.find_leds(c.image, K, D, roi=discs.roi, **discs.prm)
    assert dc.same_bits(want[0], u_ref) and dc.same_bits(want[1], d_ref)
    assert_bytes(res[0], want, "discs before")
    assert_bytes(res[2], want, "discs after")
    assert res[1][2] == sc.single("cap_b_8256")[2] == {"n": 0, "n_components": 8256, "overflow": 1}
    d = dc.case("cap_d_1225")
    corner = dc.Case("corner", "cap", d.image_id, d.image, (2, 2, 51, 45), d.prm)
    cs = [d, corner]
    res = sc.eng.find_leds_multi(d.image, rois=[e.roi for e in cs], D=D, params=[e.prm for e in cs])
    assert_bytes(res[0], sc.single("cap_d_1225"), "lattice of 1225")
    assert res[0][2]["n"] == 1225 and len(res[0][0]) == 1024
    want = sc.eng.find_leds(d.image, D=D, roi=corner.roi, **corner.prm)
    assert want[2]["n"] >= 30 and want[2]["overflow"] == 0
    assert_bytes(res[1], want, "corner")
    u_ref, d_ref, _, _ = orc.find_leds(d.image, K, D, roi=corner.roi, **corner.prm)
    assert dc.same_bits(want[0], u_ref) and dc.same_bits(want[1], d_ref)
