"""The LED detector's case suite without a GPU (tests/detect_cases.py; the GPU side is tests/test_gpu_detect_cases.py).

Two things are settled here.  The oracle (oracle/detect_oracle.cpp) is held to a yardstick written by other means: for
every case its mask equals detect_cases.numpy_mask (numpy integer arithmetic, closed-form reflection) and its
component count equals detect_cases.components (a flood fill).  And no case is vacuous: what a case is there for
(Case.want) is checked from the oracle and that mask alone: detections where they are claimed, the spiral larger than
the tracing window, the comb's teeth in several tiles, a set pixel pair across the named tile edge in the named
direction, a sparse 64 x 64 noise ROI, the symmetric shapes' centres."""
import numpy as np
import pytest

import detect_cases as dc

TILE = dc.TILE


@pytest.mark.parametrize("name", dc.names())
def test_oracle_mask_and_components_match_the_yardstick(name):
    mask, n_comp, _ = dc.yardstick(name)
    und, dist, areas, omask, stats = dc.oracle(name)
    assert omask.shape == mask.shape
    assert np.array_equal(omask.astype(bool), mask), name
    assert stats["n_components"] == n_comp, (name, stats, n_comp)
    assert not mask[0].any() and not mask[-1].any() and not mask[:, 0].any() and not mask[:, -1].any()
    assert len(und) == len(dist) == min(stats["n"], dc.MAX_BLOBS) and stats["n"] <= n_comp


@pytest.mark.parametrize("name", dc.names())
def test_case_does_what_it_is_there_for(name):
    c = dc.case(name)
    mask, n_comp, lab = dc.yardstick(name)
    und, dist, areas, _, stats = dc.oracle(name)
    w = c.want
    h, wd = mask.shape
    if "n" in w:
        assert stats["n"] == w["n"], (name, stats)
    if "n_min" in w:
        assert stats["n"] >= max(w["n_min"], 1), (name, stats)
    if "n_components" in w:
        assert n_comp == w["n_components"], (name, n_comp)
    if "n_components_min" in w:
        assert n_comp >= w["n_components_min"], (name, n_comp)
    if "overflow" in w:
        assert (n_comp > dc.MAX_COMPONENTS) == bool(w["overflow"]), (name, n_comp)
    if c.group == "zoo":
        # some link of the drawing crosses a tile border (the translates move theirs on and off the borders)
        x, y, rw, rh = c.rect
        assert mask.sum() > 0
        ys, xs = np.nonzero(mask)
        crosses = False
        for py, px in zip(ys, xs):
            for ddx, ddy in ((-1, 0), (-1, -1), (0, -1), (1, -1)):
                qx, qy = px + ddx, py + ddy
                if mask[qy, qx] and (qx // TILE != px // TILE or qy // TILE != py // TILE):
                    crosses = True
        assert crosses or name.startswith(("zoo_pixel", "zoo_hline", "zoo_vline")), name
    if w.get("spiral"):
        ys, xs = np.nonzero(lab == 0)
        first_x = xs[ys == ys.min()].min()
        assert xs.max() - xs.min() + 1 > 64 and ys.max() - ys.min() + 1 > 64   # larger than the tracing window
        assert first_x - xs.min() > 31                                         # and left of the window's first column
        assert stats["longest_contour"] > 2000
    if w.get("comb"):
        ys, xs = np.nonzero(mask)
        top = ys.min()
        n_teeth, tl = dc.components(mask[:top + TILE + 1])   # the rows down to one tile below the tops: no base there
        tiles = {int(np.nonzero(tl == t)[1].min()) // TILE for t in range(n_teeth)}
        assert n_teeth >= 4 and len(tiles) >= 3, (n_teeth, tiles)
        assert lab[top, xs[ys == top].min()] == 0 and xs[ys == top].min() - xs.min() <= 2   # the root: the first tooth
    for seam in w.get("seams", ()):
        kind, px, py = dc.seam_pixel(seam)
        ddx, ddy = {"W": (-1, 0), "N": (0, -1), "NW": (-1, -1), "NE": (1, -1)}[kind.split("_")[0]]
        qx, qy = px + ddx, py + ddy
        assert mask[py, px] and mask[qy, qx], (name, seam)
        left, top, right = px % TILE == 0, py % TILE == 0, px % TILE == TILE - 1
        where = {"W": left, "N": top, "NW_corner": left and top, "NW_left": left and not top,
                 "NW_top": top and not left, "NE_corner": right and top, "NE_right": right and not top,
                 "NE_top": top and not right}[kind]
        assert where, (name, seam)
        assert (qx // TILE, qy // TILE) != (px // TILE, py // TILE)
        if w.get("diagonal_only"):   # no 4-connected way round: the diagonal link alone joins the two tiles' pixels
            assert not mask[py, qx] and not mask[qy, px], (name, seam)
    if "thin_cols" in w:
        for col in w["thin_cols"]:
            assert mask[:, col].sum() == 1, (name, col)
    if "centre" in w:
        x, y, _, _ = c.rect
        cx, cy = w["centre"]
        assert dist.shape == (1, 2)
        assert dist[0, 0] == np.float32(cx + x) and dist[0, 1] == np.float32(cy + y), (name, dist, w["centre"])
        ys, xs = np.nonzero(mask)
        assert xs.min() + xs.max() == 2 * cx and ys.min() + ys.max() == 2 * cy   # the mask is centred there too
        box = mask[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        assert np.array_equal(box, box[::-1, ::-1])                             # and is its own half turn
    if w.get("sparse"):
        assert 1 <= n_comp <= 40, (name, n_comp)
    if w.get("frame"):
        x, y, rw, rh = c.rect
        raw = c.image[y:y + rh, x:x + rw]
        assert raw[0].any() and raw[-1].any() and raw[:, 0].any() and raw[:, -1].any()   # drawn on the frame itself
    if w.get("band"):
        x, y, rw, rh = c.rect
        assert (c.image[y - 1, x - 1:x + rw + 1] == 255).all() and (c.image[y + rh, x - 1:x + rw + 1] == 255).all()
        assert (c.image[y - 1:y + rh + 1, x - 1] == 255).all() and (c.image[y - 1:y + rh + 1, x + rw] == 255).all()
        plain = dc.Case("plain", "sweep", "noise", dc.case("sw_whole_s0.6_a1").image, c.roi, c.prm)
        assert np.array_equal(dc.numpy_mask(plain), mask)   # the same ROI without the band gives the same mask


def test_the_tables_cover_what_they_name():
    """The sweep's sides, offsets, sigmas, polarities and thresholds; the translates' shifts; the groups' sizes."""
    sweep = dc.cases("sweep")
    pairs = {(c.rect[2], c.rect[3]) for c in sweep if c.roi is not None}
    assert len(pairs) >= 24 and {(1, 1), (1, 65), (65, 1), (17, 33), (64, 64)} <= pairs
    sides = {s for p in pairs for s in p}
    assert {1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65} <= sides
    assert all(c.roi[0] % 2 == 1 and c.roi[1] % 2 == 1 for c in sweep if c.roi is not None)
    assert any(c.roi is None for c in sweep)
    for sigma in dc.SIGMAS:
        for active in (0, 1):
            assert any(c.prm["gaussian_sigma"] == sigma and c.prm["active_markers"] == active and
                       min(c.rect[2:]) <= 3 for c in sweep), (sigma, active)   # radius 15 against sides down to 1
    assert {0, 254, 255} <= {c.prm["threshold_value"] for c in sweep}
    assert int(dc.taps_q8(5.0).size) == 31 and list(dc.taps_q8(0.6)) == [1, 42, 170, 42, 1]
    assert list(dc.taps_q8(0.3)) == [1, 254, 1]
    tr = dc.cases("translate")
    assert len(tr) == 3 * len(dc.SHIFTS) ** 2
    for c in tr:
        assert c.rect[0] >= 0 and c.rect[1] >= 0
    for c in dc.cases():
        x, y, w, h = c.rect
        assert x >= 0 and y >= 0 and x + w <= c.image.shape[1] and y + h <= c.image.shape[0], c.name
        assert c.image.shape[1] <= 260 and c.image.shape[0] <= 220, c.name
    for b in dc.batches(dc.names("zoo") + dc.names("translate") + dc.names("sweep")):
        assert 1 <= len(b) <= 64 and len({dc.case(n).image_id for n in b}) == 1


def test_nan_centres_are_the_zero_area_contours():
    """Where a centre is NaN, the contour's area is zero (a one-pixel-wide diagonal walked there and back): the only
    place where same_bits lets two bit patterns pass for one."""
    seen = 0
    for name in dc.names():
        und, dist, areas, _, _ = dc.oracle(name)
        bad = np.isnan(dist).any(axis=1)
        assert np.array_equal(bad, np.isnan(und).any(axis=1))
        assert np.all(areas[bad] == 0.0), name
        seen += int(bad.sum())
    assert seen >= 6
    a = np.array([[np.nan, 1.0]])
    assert dc.same_bits(a, -a * -1.0) and not dc.same_bits(np.array([[0.0]]), np.array([[-0.0]]))
    assert not dc.same_bits(a, np.array([[1.0, 1.0]])) and not dc.same_bits(a, a.astype(np.float32))


def test_padded_views():
    img = dc.case("sw_whole_s0.6_a1").image
    for extra in (1, 37):
        p = dc.padded(img, extra)
        assert p.strides[0] == img.shape[1] + extra and np.array_equal(p, img)
        assert (p.base[:, img.shape[1]:] == 255).all()
