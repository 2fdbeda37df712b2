"""Host side of the batched LED detector (pfmpe_find_leds_multi, pfmpe_host_grow_roi): the binding's symbol list,
the array strides of the batch (sizeof the parameter and output records) and the reference's ROI enlargement
(pose_estimator.cpp:429-432 / 454-457) against known answers and a restatement.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

W, H = 752, 480


def test_symbols_are_listed():
    assert "pfmpe_find_leds_multi" in _capi.EXPORTED_SYMBOLS
    assert "pfmpe_host_grow_roi" in _capi.EXPORTED_SYMBOLS
    assert _capi.DETECT_MAX_ROIS == 64


def test_record_sizes_are_the_batch_strides():
    # 2 int32, 5 doubles, 5 doubles (D), 4 int32; 4 int32
    assert C.sizeof(_capi.DetectParams) == 8 + 5 * 8 + 5 * 8 + 16 == 104
    assert C.sizeof(_capi.DetectOut) == 16


@pytest.mark.parametrize("roi, margin, want", [
    ((375, 187, 110, 127), 20, (355, 167, 150, 167)),
    ((5, 8, 100, 50), 20, (0, 0, 140, 90)),        # x, y clamp at 0; w, h still grow by 2 * margin
    ((700, 440, 52, 40), 20, (680, 420, 72, 60)),  # w, h clipped against the moved x, y
    ((375, 187, 110, 127), 0, (375, 187, 110, 127)),
    ((0, 0, W, H), 0, (0, 0, W, H)),
])
def test_grow_roi_known_answers(roi, margin, want):
    assert pf.host_grow_roi(roi, margin, W, H) == want


def restated(roi, m, w, h):
    x, y = max(roi[0] - m, 0), max(roi[1] - m, 0)
    return (x, y, min(roi[2] + 2 * m, w - x), min(roi[3] + 2 * m, h - y))


def test_grow_roi_matches_restatement():
    rng = np.random.default_rng(454)
    for _ in range(400):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        roi = (x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1)))
        m = int(rng.integers(0, 60))
        got = pf.host_grow_roi(roi, m, W, H)
        assert got == restated(roi, m, W, H), (roi, m)
        assert got[0] >= 0 and got[1] >= 0 and got[0] + got[2] <= W and got[1] + got[3] <= H


def test_grow_roi_rejects_bad_arguments():
    lib = pf.load()
    roi = (C.c_int32 * 4)(10, 10, 20, 20)
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert lib.pfmpe_host_grow_roi(None, 20, W, H, out) == pf.E_ARG
    assert lib.pfmpe_host_grow_roi(roi, 20, W, H, None) == pf.E_ARG
    assert lib.pfmpe_host_grow_roi(roi, -1, W, H, out) == pf.E_ARG
    assert lib.pfmpe_host_grow_roi(roi, 20, 0, H, out) == pf.E_ARG
    assert lib.pfmpe_host_grow_roi(roi, 20, W, 0, out) == pf.E_ARG
    assert list(out) == [-7] * 4
    with pytest.raises(pf.PFError):
        pf.host_grow_roi((10, 10, 20, 20), -1, W, H)
