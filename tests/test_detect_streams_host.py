"""Host side of the multi-camera LED detector (pfmpe_find_leds_streams): the binding's symbols and record sizes, and
the upload plan and pack (pfmpe_host_detect_plan / pfmpe_host_detect_pack) against known answers, a Python
restatement of the rules over random batches, the plan's invariants, and the error cases.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

W, H = 752, 480
ROI_A, ROI_A20 = (375, 187, 110, 127), (355, 167, 150, 167)


def al(x, a):
    return (x + a - 1) // a * a


def test_symbols_and_sizes():
    for name in ("pfmpe_find_leds_streams", "pfmpe_host_detect_plan", "pfmpe_host_detect_pack"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(pf.load(), name)
    assert C.sizeof(_capi.DetectImage) == 32
    assert C.sizeof(_capi.DetectCrop) == 16
    assert _capi.DETECT_MAX_IMAGES == 64 == pf.DETECT_MAX_IMAGES


# ---------------------------------------------------------------------------------------------- known answers
@pytest.fixture(scope="module")
def big():
    return np.random.default_rng(1).integers(0, 256, size=(H, W), dtype=np.uint8)


def test_plan_enlarged_roi_shares_the_crop(big):
    crops, nbytes = pf.host_detect_plan([big], [0, 0], [ROI_A, ROI_A20])
    assert crops[1] == (0, 160, -1)
    assert crops[0] == (20 * 160 + 20, 160, 1) == (3220, 160, 1)
    assert nbytes == al(167 * 160, 256) == 26880


def test_plan_same_rectangle_twice_lower_index_owns(big):
    crops, nbytes = pf.host_detect_plan([big], [0, 0, 0], [ROI_A, ROI_A, ROI_A])
    assert crops[0] == (0, 112, -1)
    assert crops[1] == crops[2] == (0, 112, 0)
    assert nbytes == al(127 * 112, 256)


def test_plan_chain_shares_with_the_whole_image(big):
    crops, nbytes = pf.host_detect_plan([big], [0, 0, 0], [ROI_A, ROI_A20, None])
    assert crops[2] == (0, 752, -1)
    assert crops[0] == (187 * 752 + 375, 752, 2)
    assert crops[1] == (167 * 752 + 355, 752, 2)
    assert nbytes == al(480 * 752, 256)


def test_plan_same_rectangle_on_two_images(big):
    other = big[::-1].copy()
    crops, nbytes = pf.host_detect_plan([big, other], [0, 1], [ROI_A, ROI_A])
    assert crops[0] == (0, 112, -1)
    assert crops[1] == (al(127 * 112, 256), 112, -1) == (14336, 112, -1)
    assert nbytes == 14336 + al(127 * 112, 256)


def test_plan_staged_image(big):
    crops, nbytes = pf.host_detect_plan([(H, W), big], [0, 1, 0], [ROI_A, ROI_A, None])
    assert crops[0] == (-1, W, -1) and crops[2] == (-1, W, -1)
    assert crops[1] == (0, 112, -1)
    assert nbytes == al(127 * 112, 256)
    crops, nbytes = pf.host_detect_plan([(H, W)], [0], [ROI_A])
    assert crops == [(-1, W, -1)] and nbytes == 0


# ---------------------------------------------------------------------------------------------- restatement
def rect(roi, w, h):
    return (0, 0, w, h) if roi is None else roi


def inside(o, r):
    return o[0] <= r[0] and o[1] <= r[1] and o[0] + o[2] >= r[0] + r[2] and o[1] + o[3] >= r[1] + r[3]


def restated_plan(shapes, staged, image_of, rois):
    """The rules of the upload plan, stated again: -> (crops, upload_bytes, owner per entry)."""
    R = len(rois)
    rc = [rect(rois[r], shapes[image_of[r]][1], shapes[image_of[r]][0]) for r in range(R)]
    owner, crops, end = [None] * R, [None] * R, 0
    for r in range(R):
        if staged[image_of[r]]:
            owner[r], crops[r] = -1, (-1, shapes[image_of[r]][1], -1)
            continue
        cands = [q for q in range(R) if image_of[q] == image_of[r] and inside(rc[q], rc[r])]
        owner[r] = min(cands, key=lambda q: (-rc[q][2] * rc[q][3], q))
    for r in range(R):
        if owner[r] == r:
            pitch = al(rc[r][2], 16)
            crops[r] = (end, pitch, -1)
            end = al(end + rc[r][3] * pitch, 256)
    for r in range(R):
        q = owner[r]
        if q >= 0 and q != r:
            crops[r] = (crops[q][0] + (rc[r][1] - rc[q][1]) * crops[q][1] + rc[r][0] - rc[q][0], crops[q][1], q)
    return crops, end, owner, rc


def random_batch(rng):
    """I <= 6 images with sides 1 .. 200 and pitch >= width (some staged), R <= 64 entries; nested, repeated and
    whole-image rectangles are frequent."""
    n_img = int(rng.integers(1, 7))
    images, shapes, staged = [], [], []
    for _ in range(n_img):
        h, w = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        shapes.append((h, w))
        if rng.random() < 0.2:
            images.append((h, w))
            staged.append(True)
        else:
            full = rng.integers(0, 256, size=(h, w + int(rng.integers(0, 9))), dtype=np.uint8)
            images.append(full[:, :w])  # pitch >= width
            staged.append(False)
    R = int(rng.integers(1, 65))
    image_of, rois = [], []
    for r in range(R):
        i = int(rng.integers(0, n_img))
        h, w = shapes[i]
        kind = rng.random()
        if kind < 0.1:
            roi = None
        elif kind < 0.3 and r > 0:
            q = int(rng.integers(0, r))  # a copy of an earlier entry, or a rectangle inside it
            i = image_of[q]
            h, w = shapes[i]
            x, y, rw, rh = rect(rois[q], w, h)
            if rng.random() < 0.5:
                dx, dy = int(rng.integers(0, rw)), int(rng.integers(0, rh))
                roi = (x + dx, y + dy, int(rng.integers(1, rw - dx + 1)), int(rng.integers(1, rh - dy + 1)))
            else:
                roi = (x, y, rw, rh)
        else:
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
            roi = (x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1)))
        image_of.append(i)
        rois.append(roi)
    return images, shapes, staged, image_of, rois


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(452)
    return [random_batch(rng) for _ in range(400)]


def test_plan_matches_restatement_and_invariants(batches):
    n_shared = n_staged = 0
    for images, shapes, staged, image_of, rois in batches:
        crops, nbytes = pf.host_detect_plan(images, image_of, rois)
        want, end, owner, rc = restated_plan(shapes, staged, image_of, rois)
        assert crops == want
        assert nbytes == end
        own = [r for r in range(len(rois)) if owner[r] == r]
        spans = [(crops[r][0], crops[r][0] + rc[r][3] * crops[r][1]) for r in own]
        assert all(a % 256 == 0 for a, _ in spans)
        assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1))  # disjoint, ascending
        assert nbytes == (al(spans[-1][1], 256) if spans else 0)
        for r, q in enumerate(owner):
            if q >= 0:
                assert owner[q] == q and inside(rc[q], rc[r]) and image_of[q] == image_of[r]
        n_shared += sum(1 for r, q in enumerate(owner) if q >= 0 and q != r)
        n_staged += sum(1 for q in owner if q < 0)
    assert n_shared > 400 and n_staged > 400  # the batches exercise both


def test_pack_holds_every_entrys_pixels_and_zeros_elsewhere(batches):
    for images, shapes, staged, image_of, rois in batches:
        crops, nbytes = pf.host_detect_plan(images, image_of, rois)
        buf = pf.host_detect_pack(images, image_of, rois)
        assert buf.size == nbytes
        covered = np.zeros(nbytes, dtype=bool)
        for r, (off, pitch, shared) in enumerate(crops):
            if off < 0:
                continue
            h, w = shapes[image_of[r]]
            x, y, rw, rh = rect(rois[r], w, h)
            idx = off + np.arange(rh)[:, None] * pitch + np.arange(rw)[None, :]
            assert idx.max() < nbytes
            np.testing.assert_array_equal(buf[idx], images[image_of[r]][y:y + rh, x:x + rw])
            if shared < 0:
                covered[idx] = True
        assert not buf[~covered].any()


def test_pack_writes_all_padding(big):
    """A buffer pre-filled with a sentinel: every byte of [0, upload_bytes) is written, nothing beyond it."""
    ims, keep, ps, idx, R = _capi._host_detect_batch([big, big[:, :100]], [0, 1, 0], [ROI_A, (3, 5, 33, 17), ROI_A20])
    crops = (_capi.DetectCrop * R)()
    nbytes = C.c_int64()
    lib = pf.load()
    assert lib.pfmpe_host_detect_plan(ims, 2, idx, ps, R, crops, C.byref(nbytes)) == pf.OK
    buf = np.full(nbytes.value + 64, 0xAB, dtype=np.uint8)
    assert lib.pfmpe_host_detect_pack(ims, 2, idx, ps, R, crops, buf.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      buf.size) == pf.OK
    assert np.all(buf[nbytes.value:] == 0xAB)
    np.testing.assert_array_equal(buf[:nbytes.value], pf.host_detect_pack([big, big[:, :100]], [0, 1, 0],
                                                                          [ROI_A, (3, 5, 33, 17), ROI_A20]))
    own = {1: (0, 48, 33, 17), 2: (al(17 * 48, 256), 160, 150, 167)}
    covered = np.zeros(nbytes.value, dtype=bool)
    for r, (off, pitch, w, h) in own.items():
        assert (crops[r].offset, crops[r].pitch, crops[r].shared_with) == (off, pitch, -1)
        covered[off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :]] = True
    assert not buf[:nbytes.value][~covered].any()


# ---------------------------------------------------------------------------------------------- errors
def raw_batch(images, image_of, rois):
    ims, keep, ps, idx, R = _capi._host_detect_batch(images, image_of, rois)
    return ims, keep, ps, idx, R


def bad_batches(big):
    """(name, images, I, image_of, rois, code): the geometric error cases shared by the plan, the pack and the
    device call."""
    grid = [(10 * (i % 8), 10 * (i // 8), 9, 9) for i in range(65)]
    return [
        ("I < 1", [big], 0, [0], [ROI_A], pf.E_ARG),
        ("image index too large", [big], 1, [0, 1], [ROI_A, ROI_A], pf.E_ARG),
        ("image index negative", [big], 1, [-1], [ROI_A], pf.E_ARG),
        ("roi past the right edge", [big], 1, [0, 0], [ROI_A, (700, 440, 53, 40)], pf.E_ARG),
        ("roi with a negative corner", [big], 1, [0], [(-1, 0, 10, 10)], pf.E_ARG),
        ("roi of zero width", [big], 1, [0], [(5, 5, 0, 10)], pf.E_ARG),
        ("R > 64", [big], 1, [0] * 65, grid, pf.E_CAP),
        ("I > 64", [big] * 65, 65, [0], [ROI_A], pf.E_CAP),
    ]


def test_plan_errors_leave_outputs_untouched(big):
    lib = pf.load()
    for name, images, n_img, image_of, rois, code in bad_batches(big):
        ims, keep, ps, idx, R = raw_batch(images, image_of, rois)
        crops = (_capi.DetectCrop * max(R, 1))(*[_capi.DetectCrop(-77, -77, -77)] * max(R, 1))
        nbytes = C.c_int64(-77)
        assert lib.pfmpe_host_detect_plan(ims, n_img, idx, ps, R, crops, C.byref(nbytes)) == code, name
        assert nbytes.value == -77 and all((c.offset, c.pitch, c.shared_with) == (-77, -77, -77) for c in crops), name
    ims, keep, ps, idx, R = raw_batch([big], [0], [ROI_A])
    crops = (_capi.DetectCrop * 1)(_capi.DetectCrop(-77, -77, -77))
    nbytes = C.c_int64(-77)
    calls = {
        "R < 1": lambda: lib.pfmpe_host_detect_plan(ims, 1, idx, ps, 0, crops, C.byref(nbytes)),
        "null images": lambda: lib.pfmpe_host_detect_plan(None, 1, idx, ps, 1, crops, C.byref(nbytes)),
        "null image_of": lambda: lib.pfmpe_host_detect_plan(ims, 1, None, ps, 1, crops, C.byref(nbytes)),
        "null params": lambda: lib.pfmpe_host_detect_plan(ims, 1, idx, None, 1, crops, C.byref(nbytes)),
        "null crops": lambda: lib.pfmpe_host_detect_plan(ims, 1, idx, ps, 1, None, C.byref(nbytes)),
        "null upload_bytes": lambda: lib.pfmpe_host_detect_plan(ims, 1, idx, ps, 1, crops, None),
    }
    for field, value in (("width", 0), ("height", 0), ("pitch", W - 1)):
        def call(field=field, value=value):
            old = getattr(ims[0], field)
            setattr(ims[0], field, value)
            try:
                return lib.pfmpe_host_detect_plan(ims, 1, idx, ps, 1, crops, C.byref(nbytes))
            finally:
                setattr(ims[0], field, old)
        calls["bad image " + field] = call
    for name, call in calls.items():
        assert call() == pf.E_ARG, name
        assert nbytes.value == -77 and (crops[0].offset, crops[0].pitch, crops[0].shared_with) == (-77, -77, -77), name
    assert lib.pfmpe_host_detect_plan(ims, 1, idx, ps, 1, crops, C.byref(nbytes)) == pf.OK  # the batch itself is fine


def test_pack_errors_leave_the_buffer_untouched(big):
    lib = pf.load()
    buf = np.full(1 << 16, 0xAB, dtype=np.uint8)
    bp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    for name, images, n_img, image_of, rois, code in bad_batches(big):
        ims, keep, ps, idx, R = raw_batch(images, image_of, rois)
        crops = (_capi.DetectCrop * max(R, 1))()
        assert lib.pfmpe_host_detect_pack(ims, n_img, idx, ps, R, crops, bp, buf.size) == code, name
        assert np.all(buf == 0xAB), name
    rois = [ROI_A, ROI_A20]
    ims, keep, ps, idx, R = raw_batch([big], [0, 0], rois)
    plan, nbytes = pf.host_detect_plan([big], [0, 0], rois)
    good = (_capi.DetectCrop * 2)(*[_capi.DetectCrop(*c) for c in plan])
    moved = (_capi.DetectCrop * 2)(*[_capi.DetectCrop(*c) for c in plan])
    moved[1].offset = 256  # not the batch's plan: the pack does not write where it is told
    cases = {
        "buffer too small": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, good, bp, nbytes - 1), pf.E_CAP),
        "negative size": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, good, bp, -1), pf.E_ARG),
        "crops not the plan": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, moved, bp, buf.size), pf.E_ARG),
        "null crops": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, None, bp, buf.size), pf.E_ARG),
        "null buffer": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, good, None, buf.size), pf.E_ARG),
        "R < 1": (lambda: lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 0, good, bp, buf.size), pf.E_ARG),
    }
    for name, (call, code) in cases.items():
        assert call() == code, name
        assert np.all(buf == 0xAB), name
    with pytest.raises(pf.PFError) as ei:
        pf.host_detect_pack([big], [0, 0], rois, buffer_bytes=nbytes - 1)
    assert ei.value.code == pf.E_CAP
    assert lib.pfmpe_host_detect_pack(ims, 1, idx, ps, 2, good, bp, nbytes) == pf.OK
    assert np.all(buf[nbytes:] == 0xAB) and not np.all(buf[:nbytes] == 0xAB)
