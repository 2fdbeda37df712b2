"""Inputs of the LED detector's case suite (tests/test_detect_cases_host.py, tests/test_gpu_detect_cases.py), and the
yardstick that does not come from the oracle.

A case is (image, roi, params) for pfmpe_find_leds.  Four groups:
  zoo        shapes the border follower and the labelling have to get right (concave turns, 1-pixel bridges, diagonal
             links, contours larger than the 64 x 64 tracing window), each laid so that its critical feature sits on
             the corner of four 32 x 32 labelling tiles of its ROI (ROI-local x, y = 31 | 32)
  translate  three of those shapes moved over (dx, dy) in {0, 1, 15, 16, 31}^2 inside their ROI
  sweep      ROI sides on and around the 16 / 32 / 64 pixel tile edges over one noise image, every blur radius against
             every side, both marker polarities, the extreme thresholds
  cap        the component cap (8192) and the output cap (PFMPE_MAX_BLOBS) reached and exceeded

Three ways of drawing.  "bright": value 255 under the default threshold 240; sigma 0.6 grows a shape by about two
pixels.  "dim": value 2 under threshold 1; the taps at sigma 0.6 are [1, 42, 170, 42, 1], so an isolated pixel gives
(2 * 170 * 170 + 2^15) >> 16 = 1 and its neighbour (2 * 170 * 42 + 2^15) >> 16 = 0: lines stay one pixel wide, but a
hole with three or four set 4-neighbours fills (3 * 14280 + 2^15 >= 2^16).  "exact": value 30 under threshold 10 at
sigma 0.3, taps [1, 254, 1]; a set pixel gives 30 * 254 * 254 >> 16 > 0 and an unset one at most
4 * 30 * 254 + 4 * 30 = 30600 < 2^15, so the mask is the drawing, whatever the drawing.

The yardstick: numpy_mask() restates the mask stage in numpy integer arithmetic and components() counts 8-connected
components by a flood fill; neither shares code with oracle/detect_oracle.cpp or the kernels.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

K, D = syn.K_README, syn.D_README
TILE = 32
MAX_BLOBS = 1024        # PFMPE_MAX_BLOBS
MAX_COMPONENTS = 8192   # components examined per ROI
LOOSE = {"min_blob_area": 0.0, "max_blob_area": 1e18, "max_circular_distortion": 1e18,
         "max_width_height_distortion": 10.0}
BRIGHT = {**LOOSE}                                                        # value 255
DIM = {**LOOSE, "threshold_value": 1}                                     # value 2
EXACT = {**LOOSE, "threshold_value": 10, "gaussian_sigma": 0.3}           # value 30
VALUE = {"bright": 255, "dim": 2, "exact": 30}
PARAMS = {"bright": BRIGHT, "dim": DIM, "exact": EXACT}
SHIFTS = (0, 1, 15, 16, 31)
CANVAS_W, CANVAS_H = 256, 216


@dataclass
class Case:
    name: str
    group: str            # zoo | translate | sweep | cap
    image_id: str         # cases with the same image_id share `image` (one find_leds_multi batch can hold them)
    image: np.ndarray
    roi: tuple | None     # (x, y, w, h); None: the whole image
    prm: dict             # fields of pfmpe_detect_params away from their defaults
    want: dict = field(default_factory=dict)  # what the case is there for (test_detect_cases_host.py checks it)

    @property
    def rect(self):
        return self.roi if self.roi is not None else (0, 0, self.image.shape[1], self.image.shape[0])


# ------------------------------------------------------------------ the yardstick that is not the oracle
def taps_q8(sigma: float) -> np.ndarray:
    """getGaussianKernel(cvRound(6 sigma + 1) | 1, sigma, CV_32F) as integers with 8 fraction bits."""
    n = int(np.rint(sigma * 3 * 2 + 1)) | 1
    x = np.arange(n) - (n - 1) * 0.5
    cf = np.exp(-0.5 / (sigma * sigma) * x * x).astype(np.float32)
    total = 0.0
    for c in cf:
        total += float(c)
    cf = (cf.astype(np.float64) * (1.0 / total)).astype(np.float32)
    return np.rint(cf.astype(np.float64) * 256.0).astype(np.int64)


def reflect101(p: np.ndarray, n: int) -> np.ndarray:
    """BORDER_REFLECT_101 of the indices p into 0 .. n-1 (closed form: the pattern has period 2 (n - 1))."""
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * (n - 1))
    return np.where(q >= n, 2 * (n - 1) - q, q)


def numpy_mask(case: Case) -> np.ndarray:
    """The detector's mask of the case's ROI (bool, h x w): threshold, integer row and column pass over the
    reflect-101 padded ROI, (s + 2^15) >> 16 > 0, the 1-pixel frame cleared."""
    x, y, w, h = case.rect
    prm = case.prm
    thr, active = prm.get("threshold_value", 240), prm.get("active_markers", 1)
    v = case.image[y:y + h, x:x + w].astype(np.int64)
    t = np.where(v > thr, v, 0) if active else np.where(v > thr, 0, 255)
    k = taps_q8(prm.get("gaussian_sigma", 0.6))
    r = len(k) // 2
    ix, iy = reflect101(np.arange(-r, w + r), w), reflect101(np.arange(-r, h + r), h)
    rows = sum(int(k[i]) * t[:, ix[i:i + w]] for i in range(len(k)))
    cols = sum(int(k[i]) * rows[iy[i:i + h], :] for i in range(len(k)))
    m = ((cols + (1 << 15)) >> 16) > 0
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    return m


def components(mask: np.ndarray):
    """8-connected components by flood fill -> (count, labels h x w int32: -1 off, else the component's number in
    raster order of its first pixel)."""
    h, w = mask.shape
    lab = np.full((h, w), -1, dtype=np.int32)
    on = mask.tolist()
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if lab[y0, x0] >= 0:
            continue
        lab[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            cy, cx = stack.pop()
            for ny in range(max(cy - 1, 0), min(cy + 2, h)):
                row = on[ny]
                for nx in range(max(cx - 1, 0), min(cx + 2, w)):
                    if row[nx] and lab[ny, nx] < 0:
                        lab[ny, nx] = n
                        stack.append((ny, nx))
        n += 1
    return n, lab


@functools.lru_cache(maxsize=None)
def yardstick(name: str):
    """(mask, component count, labels) of the case, from numpy_mask and components (once per case)."""
    m = numpy_mask(case(name))
    n, lab = components(m)
    m.setflags(write=False)
    lab.setflags(write=False)
    return m, n, lab


@functools.lru_cache(maxsize=None)
def oracle(name: str, max_out: int = MAX_BLOBS):
    """oracle/detect_oracle.cpp on the case -> (undistorted, distorted, areas, mask, stats), once per case."""
    c = case(name)
    kw = dict(c.prm)
    if "active_markers" in kw:
        kw["active_markers"] = bool(kw["active_markers"])
    res = orc.find_leds(c.image, K, D, roi=c.roi, max_out=max_out, want_mask=True, want_stats=True, **kw)
    for a in res[:4]:
        a.setflags(write=False)
    return res


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Same shape, same type, every number the same bits.  A zero-area contour that the loose filters keep has the
    centre 0 / 0: NaN on either side, whose sign and payload are the platform's and say nothing; a NaN matches a NaN
    in the same place."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ drawing
def _line(a, p, q):
    """Inclusive segment p -> q (x, y), axis-aligned or at 45 degrees."""
    (x0, y0), (x1, y1) = p, q
    n = max(abs(x1 - x0), abs(y1 - y0))
    sx, sy = int(np.sign(x1 - x0)), int(np.sign(y1 - y0))
    for i in range(n + 1):
        a[y0 + sy * i, x0 + sx * i] = True


def _path(a, pts):
    for p, q in zip(pts, pts[1:]):
        _line(a, p, q)


def _disc(a, cx, cy, r):
    yy, xx = np.ogrid[:a.shape[0], :a.shape[1]]
    a |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def _blank(w, h):
    return np.zeros((h, w), dtype=bool)


# Every shape: (drawing, anchor).  The anchor (x, y) is the drawing's pixel that lands on ROI-local (32, 32), the first
# pixel of tile (1, 1): its W, NW, N neighbours lie in three other tiles.
def sh_spiral():
    """Square spiral 101 px across, arms 8 apart, entered in the middle of its top side: the raster-first pixel is
    (56, 0) and the outer arm comes back to x = 0."""
    a = _blank(101, 101)
    lo, hi = 0, 100
    pts = [(56, lo), (hi, lo), (hi, hi), (lo, hi)]
    while hi - lo > 24:
        pts.append((lo, lo + 8))
        lo += 8
        hi -= 8
        pts += [(hi, lo), (hi, hi), (lo, hi)]
    _path(a, pts)
    return a, (28, 28)


def sh_comb():
    """Four teeth pointing up, 33 apart, joined by a base 38 rows below their tops."""
    a = _blank(100, 39)
    for x in (0, 33, 66, 99):
        _line(a, (x, 0), (x, 38))
    _line(a, (0, 38), (99, 38))
    return a, (29, 29)


def sh_u():
    a = _blank(9, 13)
    _path(a, [(0, 0), (0, 12), (8, 12), (8, 0)])
    return a, (4, 12)


def sh_w():
    a = _blank(33, 9)
    _path(a, [(0, 0), (8, 8), (16, 0), (24, 8), (32, 0)])
    return a, (16, 0)


def sh_diag(kind):
    """A 25-pixel diagonal whose link across the tile border is the one `kind` names (det_merge_pixel's cases)."""
    a = _blank(25, 25)
    if kind.startswith("NW"):
        _line(a, (0, 0), (24, 24))
        return a, {"NW_corner": (12, 12), "NW_left": (12, 7), "NW_top": (7, 12)}[kind]
    _line(a, (24, 0), (0, 24))
    # the pixel at ROI-local (31, 32) [corner], (31, 37) [right column only], (26, 32) [top row only] has the NE link
    return a, {"NE_corner": (13, 12), "NE_right": (13, 7), "NE_top": (18, 12)}[kind]


def sh_stairs(main):
    """A 4-connected staircase along a diagonal: (i, i), (i + 1, i)."""
    a = _blank(26, 25)
    for i in range(25):
        x = i if main else 24 - i
        a[i, x] = a[i, x + 1] = True
    return a, (12, 12)


def sh_x():
    a = _blank(21, 21)
    _line(a, (0, 0), (20, 20))
    _line(a, (20, 0), (0, 20))
    return a, (10, 10)


def sh_checker():
    a = _blank(12, 12)
    yy, xx = np.ogrid[:12, :12]
    a |= (xx + yy) % 2 == 0
    return a, (6, 6)


def sh_ring_dot():
    a = _blank(25, 25)
    _disc(a, 12, 12, 12)
    hole = _blank(25, 25)
    _disc(hole, 12, 12, 9)
    a &= ~hole
    a[12, 12] = True
    return a, (12, 12)


def sh_dumbbell():
    a = _blank(31, 11)
    _disc(a, 5, 5, 5)
    _disc(a, 25, 5, 5)
    _line(a, (10, 5), (20, 5))
    return a, (15, 5)


def sh_pixel():
    return np.ones((1, 1), dtype=bool), (0, 0)


def sh_hline():
    return np.ones((1, 9), dtype=bool), (4, 0)


def sh_vline():
    return np.ones((9, 1), dtype=bool), (0, 4)


def sh_rect():
    return np.ones((7, 12), dtype=bool), (6, 3)


def sh_ring():
    a = _blank(21, 21)
    _disc(a, 10, 10, 10)
    hole = _blank(21, 21)
    _disc(hole, 10, 10, 6)
    return a & ~hole, (10, 10)


def sh_plus():
    a = _blank(15, 15)
    a[6:9, :] = True
    a[:, 6:9] = True
    return a, (7, 7)


def sh_diamond():
    yy, xx = np.ogrid[:17, :17]
    return (abs(xx - 8) + abs(yy - 8) <= 8), (8, 8)


def _patch(draw, anchor, value, dx=0, dy=0, margin=4):
    """The ROI's pixels: the drawing with its anchor on ROI-local (32 + dx, 32 + dy), at least `margin` zero pixels
    around it."""
    h, w = draw.shape
    ox, oy = TILE - anchor[0], TILE - anchor[1]
    while ox < margin:
        ox += TILE
    while oy < margin:
        oy += TILE
    ox, oy = ox + dx, oy + dy
    p = np.zeros((oy + h + margin, ox + w + margin), dtype=np.uint8)
    p[oy:oy + h, ox:ox + w][draw] = value
    return p, (ox, oy)


class _Canvases:
    """Shelf packing of patches into CANVAS_W x CANVAS_H images, a 1-pixel gap and an odd origin; an ROI reads no
    pixel outside itself, so patches may touch."""

    def __init__(self, prefix):
        self.prefix, self.images = prefix, []
        self._new()

    def _new(self):
        self.images.append(np.zeros((CANVAS_H, CANVAS_W), dtype=np.uint8))
        self.x, self.y, self.shelf = 1, 1, 0

    def place(self, patch):
        h, w = patch.shape
        assert w + 1 <= CANVAS_W and h + 1 <= CANVAS_H, (w, h)
        if self.x + w > CANVAS_W:
            self.x, self.y, self.shelf = 1, self.y + self.shelf + 1, 0
        if self.y + h > CANVAS_H:
            self._new()
        img = self.images[-1]
        img[self.y:self.y + h, self.x:self.x + w] = patch
        roi = (self.x, self.y, w, h)
        self.x += w + 1
        self.shelf = max(self.shelf, h)
        return "%s%d" % (self.prefix, len(self.images) - 1), img, roi


def seam_pixel(seam):
    """(kind, x, y) of a `seams` entry: the ROI-local pixel whose link of that kind crosses the tile border."""
    if not isinstance(seam, str):
        return seam
    return (seam,) + {"NW_corner": (32, 32), "NW_left": (32, 37), "NW_top": (37, 32),
            "NE_corner": (31, 32), "NE_right": (31, 37), "NE_top": (26, 32), "W": (32, 32), "N": (32, 32)}[seam]


def _zoo():
    cv = _Canvases("zoo")
    out = []

    def add(name, shape, mode, **want):
        draw, anchor = shape
        patch, _ = _patch(draw, anchor, VALUE[mode])
        image_id, img, roi = cv.place(patch)
        out.append(Case("zoo_%s_%s" % (name, mode), "zoo", image_id, img, roi, dict(PARAMS[mode]), want))

    # want: n_min detections at least, n / n_components exactly, seams [(kind, x, y)], centre (ROI-local, exact)
    add("spiral", sh_spiral(), "bright", n_min=1, n_components=1, spiral=True)
    add("spiral", sh_spiral(), "dim", n_min=1, n_components=1, spiral=True)
    add("comb", sh_comb(), "bright", n_min=1, n_components=1, comb=True)
    add("comb", sh_comb(), "dim", n_min=1, n_components=1, comb=True)
    for mode in ("bright", "dim"):
        add("u", sh_u(), mode, n_min=1, n_components=1, seams=["W"])
        add("w", sh_w(), mode, n_min=1, n_components=1)
        add("x", sh_x(), mode, n_min=1, n_components=1)
        add("dumbbell", sh_dumbbell(), mode, n_min=1, n_components=1, seams=["W"])
    add("x", sh_x(), "exact", n_min=1, n_components=1, seams=["NW_corner"], diagonal_only=True)
    add("dumbbell", sh_dumbbell(), "exact", n_min=1, n_components=1, seams=["W"], thin_cols=(31, 32))
    for kind in ("NW_corner", "NW_left", "NW_top", "NE_corner", "NE_right", "NE_top"):
        for mode in ("dim", "exact"):
            add("diag_" + kind, sh_diag(kind), mode, n_min=1, n_components=1, seams=[kind], diagonal_only=True)
    add("diag_NW_corner", sh_diag("NW_corner"), "bright", n_min=1, n_components=1)
    add("diag_NE_corner", sh_diag("NE_corner"), "bright", n_min=1, n_components=1)
    add("stairs_main", sh_stairs(True), "dim", n_min=1, n_components=1, seams=["N"])
    add("stairs_anti", sh_stairs(False), "dim", n_min=1, n_components=1, seams=[("W", 32, 33)])
    add("checker", sh_checker(), "exact", n_min=1, n_components=1, seams=["NW_corner"], diagonal_only=True)
    add("checker", sh_checker(), "dim", n_min=1, n_components=1)
    add("ring_dot", sh_ring_dot(), "bright", n=2, n_components=2)   # the nested component is kept
    add("ring_dot", sh_ring_dot(), "exact", n_components=2)         # the dot is one pixel: a component, no detection
    for mode in ("dim", "exact"):
        add("pixel", sh_pixel(), mode, n_components=1)
        add("hline", sh_hline(), mode, n_components=1)
        add("vline", sh_vline(), mode, n_components=1)
    for name, shape in (("rect", sh_rect()), ("ring", sh_ring()), ("plus", sh_plus()), ("diamond", sh_diamond())):
        draw, anchor = shape
        patch, (ox, oy) = _patch(draw, anchor, 255)
        image_id, img, roi = cv.place(patch)
        centre = (ox + (draw.shape[1] - 1) / 2.0, oy + (draw.shape[0] - 1) / 2.0)
        out.append(Case("zoo_sym_%s_bright" % name, "zoo", image_id, img, roi, dict(BRIGHT),
                        {"n": 1, "n_components": 1, "centre": centre}))
    # discs on the four sides and in two corners of the ROI: the cleared frame cuts them
    p = np.zeros((64, 64), dtype=np.uint8)
    t = _blank(64, 64)
    for cx, cy in ((0, 32), (63, 32), (32, 0), (32, 63), (0, 0), (63, 63)):
        _disc(t, cx, cy, 5)
    p[t] = 255
    image_id, img, roi = cv.place(p)
    out.append(Case("zoo_frame_touch_bright", "zoo", image_id, img, roi, dict(BRIGHT),
                    {"n_min": 4, "n_components": 6, "frame": True}))
    return out


def _translates():
    out = []
    for name, shape, mode in (("dumbbell", sh_dumbbell(), "exact"), ("ring_dot", sh_ring_dot(), "bright"),
                              ("x", sh_x(), "dim")):
        draw, anchor = shape
        # one drawing in the image; the ROI moves against it, so the drawing lands on ROI-local (32 + dx, 32 + dy)
        patch, (ox, oy) = _patch(draw, anchor, VALUE[mode])
        ph, pw = patch.shape
        img = np.zeros((ph + 32, pw + 32), dtype=np.uint8)
        img[:ph, :pw] = patch
        img = np.roll(np.roll(img, 31, axis=0), 31, axis=1)   # the patch at (31, 31): room for every shift
        img.setflags(write=False)
        nc = 2 if name == "ring_dot" else 1
        for dy in SHIFTS:
            for dx in SHIFTS:
                roi = (31 - dx, 31 - dy, pw + dx, ph + dy)
                out.append(Case("tr_%s_%s_%d_%d" % (name, mode, dx, dy), "translate", "tr_" + name, img, roi,
                                dict(PARAMS[mode]), {"n_min": nc if name != "x" else 1, "n_components": nc}))
    return out


# the sweep's ROI sides: on, one below and one above the 16 / 32 / 64 pixel tile edges, and the smallest
SWEEP_PAIRS = [(1, 1), (1, 65), (65, 1), (17, 33), (64, 64), (2, 2), (3, 3), (2, 33), (33, 2), (3, 17), (15, 15),
               (16, 16), (17, 17), (15, 32), (32, 15), (16, 33), (31, 31), (32, 32), (33, 33), (31, 64), (64, 31),
               (63, 63), (65, 65), (63, 17), (17, 63), (65, 33), (33, 65), (32, 3), (3, 32), (16, 1), (64, 2),
               (31, 16)]
SIGMAS = (0.6, 1.3, 5.0)
NOISE_W, NOISE_H = 150, 131
# uniform 0..255 noise: 2 of 256 values pass either way, about 30 seeds in 62 x 62 pixels
THR_ACTIVE, THR_PASSIVE = 253, 1


def _sweep():
    rng = np.random.default_rng(20240)
    noise = rng.integers(0, 256, size=(NOISE_H, NOISE_W), dtype=np.uint8)
    noise.setflags(write=False)
    out = []

    def add(name, img, image_id, roi, sigma, active, thr, **want):
        prm = {**LOOSE, "gaussian_sigma": sigma, "active_markers": active, "threshold_value": thr}
        out.append(Case(name, "sweep", image_id, img, roi, prm, want))

    for i, (w, h) in enumerate(SWEEP_PAIRS):
        x, y = 1 + 2 * ((5 * i) % 20), 3 + 2 * ((3 * i) % 15)   # odd offsets
        for s, sigma in enumerate(SIGMAS):
            active = (i + s) % 2
            want = {"sparse": True} if (w, h) == (64, 64) else {}
            if min(w, h) >= 31:
                want["n_components_min"] = 1
            add("sw_%dx%d_s%g_a%d" % (w, h, sigma, active), noise, "noise", (x, y, w, h), sigma, active,
                THR_ACTIVE if active else THR_PASSIVE, **want)
    # 64 x 64 with the other polarity at every sigma, so that both polarities are "sparse"-checked there
    for s, sigma in enumerate(SIGMAS):
        active = (4 + s + 1) % 2
        add("sw_64x64_s%g_a%d" % (sigma, active), noise, "noise", (41, 27, 64, 64), sigma, active,
            THR_ACTIVE if active else THR_PASSIVE, sparse=True)
    for j, (roi, sigma) in enumerate((((41, 27, 64, 64), 0.6), ((7, 5, 17, 33), 1.3), ((11, 9, 33, 65), 5.0))):
        for thr in (0, 254, 255):
            for active in (0, 1):
                add("sw_thr%d_a%d_%dx%d_s%g" % (thr, active, roi[2], roi[3], sigma), noise, "noise", roi, sigma,
                    active, thr)
    for sigma in SIGMAS:
        for active in (0, 1):
            add("sw_whole_s%g_a%d" % (sigma, active), noise, "noise", None, sigma, active,
                THR_ACTIVE if active else THR_PASSIVE, n_components_min=1)
    # a saturated band one pixel outside the ROI: the blur reflects the ROI and must not see it
    band = noise.copy()
    bx, by, bw, bh = 37, 41, 33, 31
    band[by - 1, bx - 1:bx + bw + 1] = band[by + bh, bx - 1:bx + bw + 1] = 255
    band[by - 1:by + bh + 1, bx - 1] = band[by - 1:by + bh + 1, bx + bw] = 255
    band.setflags(write=False)
    for sigma in SIGMAS:
        add("sw_band_s%g" % sigma, band, "band", (bx, by, bw, bh), sigma, 1, THR_ACTIVE, band=True,
            n_components_min=1)
    return out


def _lattice(w, h, nx, ny, pitch, first, value):
    img = np.zeros((h, w), dtype=np.uint8)
    img[first:first + pitch * ny:pitch, first:first + pitch * nx:pitch] = value
    img.setflags(write=False)
    return img


def _caps():
    dim = {"threshold_value": 1}   # the default filters: a one-pixel component is never a detection
    a = _lattice(257, 129, 128, 64, 2, 1, 2)
    b = _lattice(259, 129, 129, 64, 2, 1, 2)
    c = np.zeros((151, 259), dtype=np.uint8)   # (b), and five discs below the lattice: 8256 + 5 components
    c[:129] = b
    t = np.zeros(c.shape, dtype=bool)
    for cx in (20, 70, 130, 200, 240):
        _disc(t, cx, 140, 4)
    c[t] = 255
    c.setflags(write=False)
    d = _lattice(216, 216, 35, 35, 6, 5, 255)
    return [
        Case("cap_a_8192", "cap", "cap_a", a, None, dict(dim), {"n": 0, "n_components": 8192, "overflow": 0}),
        Case("cap_b_8256", "cap", "cap_b", b, None, dict(dim), {"n": 0, "n_components": 8256, "overflow": 1}),
        Case("cap_c_8256_discs", "cap", "cap_c", c, None, {"threshold_value": 1, "min_blob_area": 0.0},
             {"n": 5, "n_components": 8261, "overflow": 1}),
        Case("cap_d_1225", "cap", "cap_d", d, None, {"min_blob_area": 0.0},
             {"n": 1225, "n_components": 1225, "overflow": 0}),
    ]


@functools.lru_cache(maxsize=None)
def _all():
    cs = _zoo() + _translates() + _sweep() + _caps()
    for c in cs:
        c.image.setflags(write=False)
    by_name = {c.name: c for c in cs}
    assert len(by_name) == len(cs), "duplicate case name"
    return by_name


def cases(group=None):
    return [c for c in _all().values() if group is None or c.group == group]


def names(group=None):
    return [c.name for c in cases(group)]


def case(name: str) -> Case:
    return _all()[name]


def batches(group_names, limit=64):
    """The named cases split into find_leds_multi batches: one image each, at most `limit` entries, tiny and large
    ROIs interleaved (smallest, largest, second smallest, ...)."""
    by_image = {}
    for n in group_names:
        by_image.setdefault(case(n).image_id, []).append(n)
    out = []
    for image_id, ns in by_image.items():
        ns = sorted(ns, key=lambda n: (case(n).rect[2] * case(n).rect[3], n))
        mixed = []
        while ns:
            mixed.append(ns.pop(0))
            if ns:
                mixed.append(ns.pop())
        out += [mixed[i:i + limit] for i in range(0, len(mixed), limit)]
    return out


def padded(image: np.ndarray, extra: int) -> np.ndarray:
    """A view of the image's pixels in a buffer whose rows are `extra` bytes longer; the padding is 255, so reading
    it shows."""
    h, w = image.shape
    buf = np.full((h, w + extra), 255, dtype=np.uint8)
    buf[:, :w] = image
    return buf[:, :w]
