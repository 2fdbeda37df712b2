"""The inputs of tests/test_gpu_envelope.py, checked from the oracle alone.

The fp32 / fp16 comparisons allow a weight to differ discretely on at most 3 of the 700 particles (a marker within
~1e-5 px of the tol_PF gate may flip).  That cap is a condition on the input: here every such frame is run through the
oracle at tol_PF and at tol_PF -+ 1e-4 px, ten times the distance at which fp32 can flip a marker, and at most 3 of the
700 weights may change (at most 1 does).  Every case must also do what it is there for: run all 80 iterations, be
refused, be accepted with a duplicate blob among its pairs, ... (Inp.want).  A case that fails either check gets
another blob seed, never a wider cap.
"""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

import envelope_cases as ec

FRAMES = ec.all_fp32_frames()


def test_markers_for_rows():
    m16 = syn.markers_16()
    assert m16.shape == (16, 3)
    assert np.array_equal(m16[:12], syn.markers_12())
    for M in range(0, 17):
        m = syn.markers_for(M)
        assert m.shape == (M, 3), M
        assert np.array_equal(m, syn.MARKERS_5[:M] if M <= 5 else m16[:M]), M
    for M in (17, 32, -1):
        with pytest.raises(ValueError):
            syn.markers_for(M)


def test_case_tables():
    names = [f.name for f in FRAMES]
    assert len(set(names)) == len(names)  # the oracle cache is keyed by name
    assert {M for M, _ in ec.MARKER_CASES} == {1, 2, 3, 4, 6, 7, 8, 9, 11, 13, 15, 16}
    assert all(f.blobs.shape[0] <= pf.MAX_BLOBS and len(f.markers) <= pf.MAX_MARKERS for f in FRAMES)
    assert ec.prior().shape == (ec.N, 12)


@pytest.mark.parametrize("inp", FRAMES, ids=[f.name for f in FRAMES])
def test_frame_is_away_from_the_gate_and_not_vacuous(inp):
    prior = ec.prior_f32()
    ref, arr = ec.oracle(inp, pf.RNG_PHILOX, prior)
    tol_pf = ec.params(inp, pf.RNG_PHILOX).tol_pf
    for shift in (-1e-4, 1e-4):
        ref2, arr2 = ec.oracle(inp, pf.RNG_PHILOX, prior, tol_pf=tol_pf + shift)
        changed = int(np.sum(arr["weights"] != arr2["weights"]))
        assert changed <= 3, (shift, changed)
        assert (ref2["accepted"], ref2["iters"]) == (ref["accepted"], ref["iters"]), shift
    want = inp.want
    for k in ("iters", "flag_fail", "accepted", "resampled"):
        if k in want:
            assert ref[k] == want[k], (k, ref[k], want[k])
    w = arr["weights"]
    if want.get("zero_weights"):
        assert np.all(w == 0.0)
    if want.get("few_weights"):
        assert 0 < np.count_nonzero(w) <= ec.N // 20, np.count_nonzero(w)
    if want.get("duplicate"):  # two LEDs on one blob, a downgraded LED among the pairs, fewer blobs than LEDs
        pairs = ref["pairs"]
        assert len(set(pairs[:, 1])) < len(pairs), pairs
        assert inp.downgrade[pairs[:, 0] - 1].any() and inp.blobs.shape[0] == len(inp.markers) - 1
        plain, _ = ec.oracle(ec.Inp(**{**inp.__dict__, "downgrade": None}), pf.RNG_PHILOX, prior)
        assert plain["highest_prob"] > ref["highest_prob"]  # the downgrade penalty is in the score
    if want.get("same_pairs_as_base"):
        base, _ = ec.oracle(ec.pred_case(inp.name.split("-")[0], "base")[0], pf.RNG_PHILOX, prior)
        assert ref["n_corr"] == base["n_corr"] == min(len(inp.markers), base["n_corr"])
        assert ref["n_corr"] >= 5
    if inp.downgrade is not None:
        assert inp.downgrade.any()
    if inp.force_iters == 0 and "iters" not in want and inp.blobs.shape[0] >= len(inp.markers) >= 3 \
            and np.isfinite(inp.blobs).all() and inp.prm.get("ang_max", 0.0) < 0.1:
        assert ref["accepted"] == 1, inp.name  # a plain tracked frame
