"""GPU parity of the brute-force P3P (re)initialisation (PoseEstimator::initialise,
pf_mpe_lib/src/pose_estimator.cpp:1503-1786) through the C-ABI against the oracle.

Bars:
  * histogram (integer, PE:1526-1716): equal to the oracle's entry for entry.  Both follow the same
    fp64 operation order (-ffp-contract=off); the elementary functions inside the quartic's complex
    pow/log (glibc vs the device's ocml) are the only source of difference, at the ulp level.
  * post-histogram stages, fed the GPU's histogram: every discrete output identical (found, flag,
    candidates, first match, correspondences, number of stored P3P poses); predicted_pose_ within 1e-9;
    the seeded particle set within the state's storage precision (fp64 1e-12, fp32 4e-7 abs,
    fp16-delta 1e-3 abs).
  * a PF step after the initialisation (fp64 state, reference RNG) matches the oracle run on the
    oracle's own seeded set exactly, as tests/test_gpu_parity.py requires of any step.
"""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

pytestmark = pytest.mark.gpu
K = syn.K_README

# (M, uniform outliers, near outliers, seed, noise px)
CASES = [(5, 3, 0, 0, 0.0), (5, 10, 2, 1, 0.3), (8, 3, 0, 6, 0.0), (6, 4, 1, 9, 0.3), (5, 45, 0, 2, 0.3),
         (12, 3, 0, 3, 0.0), (12, 8, 4, 4, 0.3)]
# the M = 12 marker set is self-similar enough that its candidate vectors explode past any cap (the
# reference would enumerate millions): histogram parity only there, initialise on CASES[:4]


def engine(M, N=256, state=pf.STATE_F64, rng=pf.RNG_REFERENCE):
    eng = pf.Engine(device=0, max_particles=N, state_dtype=state)
    eng.set_model(syn.markers_for(M), K)
    prm = pf.default_params()
    prm.rng_mode = rng
    eng.set_params(prm)
    return eng


@pytest.mark.parametrize("case", CASES, ids=[f"M{c[0]}_B{c[0] + c[1] + c[2]}_s{c[3]}" for c in CASES])
def test_histogram_matches_oracle(case):
    M, n_out, near, seed, noise = case
    blobs, _ = syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)
    eng = engine(M)
    h_gpu = eng.p3p_histogram(blobs).astype(np.int64)
    h_ref, lo, hi, unbounded = orc.init_histogram_bounds(syn.markers_for(M), K, blobs, tol=5.0)
    h_ref, lo, hi = h_ref.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)
    assert h_gpu.sum() > 0
    # every decision with a margin above the ulp level is the reference's: lo <= gpu <= hi
    assert (h_gpu >= lo).all(), np.argwhere(h_gpu < lo)[:10]
    excess = np.maximum(h_gpu - hi, 0).sum()
    assert excess <= unbounded * (3 + M), (excess, unbounded)
    # and the fragile ones mostly fall the same way: <= 0.5 % of the counts differ
    assert np.abs(h_gpu - h_ref).sum() <= max(4, 0.005 * h_ref.sum()), (np.abs(h_gpu - h_ref).sum(), h_ref.sum())
    eng.close()


def test_histogram_global_atomics_path():
    """B x M x 4 bytes > 32 KB: the histogram does not fit in LDS and the block counts straight into global memory.
    M = 12 and the smallest such B, 683.  The 12 markers and 3 outliers lie in the image, the other 668 blobs on a
    line 1001 px apart, so only the C(15,3) combinations within the image pass the spread filter: the oracle takes
    about 4 s for the 5.3e7 combinations, the device a fraction of that."""
    M, B = 12, 683
    near, _ = syn.init_blobs(M, 3, seed=3)
    blobs = np.vstack([near, [[2000.0 + 1001.0 * k, 240.0] for k in range(B - len(near))]])
    assert B * M * 4 > 32 * 1024 >= (B - 1) * M * 4
    eng = engine(M)
    h_gpu = eng.p3p_histogram(blobs).astype(np.int64)
    h_ref, lo, hi, unbounded = orc.init_histogram_bounds(syn.markers_for(M), K, blobs, tol=5.0)
    h_ref, lo, hi = h_ref.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)
    assert h_gpu.sum() > 0 and not h_gpu[len(near):].any()
    assert (h_gpu >= lo).all(), np.argwhere(h_gpu < lo)[:10]
    excess = np.maximum(h_gpu - hi, 0).sum()
    assert excess <= unbounded * (3 + M), (excess, unbounded)
    assert np.abs(h_gpu - h_ref).sum() <= max(4, 0.005 * h_ref.sum()), (np.abs(h_gpu - h_ref).sum(), h_ref.sum())
    eng.close()


@pytest.mark.parametrize("state", ["f64", "f32", "f16"])
@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: f"M{c[0]}_s{c[3]}")
def test_initialise_matches_oracle(case, state):
    M, n_out, near, seed, noise = case
    st = {"f64": pf.STATE_F64, "f32": pf.STATE_F32, "f16": pf.STATE_F16}[state]
    N = 200
    blobs, T = syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)
    eng = engine(M, N, st)
    out, h = eng.initialise(blobs, n_particles=N)
    ref, h_ref, parts = orc.initialise(syn.markers_for(M), K, blobs, N, hist=h)
    for k in ("found", "flag_fail", "n_estimates", "n_candidates", "first_match", "hist_total"):
        assert out[k] == ref[k], (k, out[k], ref[k])
    assert np.array_equal(out["pairs"], ref["pairs"])
    assert out["found"] == 1
    np.testing.assert_allclose(out["predicted_pose"], ref["predicted_pose"], rtol=0, atol=1e-9)
    if near == 0:  # near-blob outliers can make the reference itself pick a wrong first match
        assert np.abs(syn.to44(out["predicted_pose"]) - T).max() < 3e-2
    got = eng.get_particles(1)
    tol = {"f64": 1e-12, "f32": 4e-7, "f16": 1e-3}[state]
    np.testing.assert_allclose(got, parts, rtol=0, atol=tol)
    eng.close()


def test_initialise_then_pf_step_matches_oracle():
    M, N = 5, 300
    blobs, T = syn.init_blobs(M, 3, 11, noise_px=0.2)
    eng = engine(M, N)
    out, h = eng.initialise(blobs, n_particles=N)
    ref, _, parts = orc.initialise(syn.markers_for(M), K, blobs, N, hist=h)
    assert out["found"] == 1
    np.testing.assert_allclose(eng.get_particles(1), parts, rtol=0, atol=1e-12)
    parts = eng.get_particles(1)  # the step is compared from the engine's own seeded set
    # next frame: the tracker hands over current = predicted = predicted_pose_ right after init
    cur = out["predicted_pose"]
    nb = syn.project(K, T, syn.markers_for(M)) + 0.3
    fr = eng.make_frame(cur, cur, np.eye(4)[:3].reshape(12), blobs=nb, it_since_init=1, dt=0.02, seed=77)
    o = eng.step(fr).as_dict()
    r, arr = orc.pf_step(syn.markers_for(M), K, orc.make_params(rng_mode=orc.RNG_REFERENCE), parts, cur, cur,
                         np.eye(4)[:3].reshape(12), nb, it_since_init=1, dt=0.02, seed=77)
    for k in ("iters", "kept_iter", "accepted", "most_likely_idx", "winner_idx", "n_corr"):
        assert o[k] == r[k], k
    np.testing.assert_allclose(eng.get_weights(), arr["weights"], rtol=0, atol=1e-9)
    eng.close()


def test_initialise_too_few_blobs_and_errors():
    eng = engine(5)
    blobs, _ = syn.init_blobs(5, 0, 0)
    out, _ = eng.initialise(blobs[:4], n_particles=100)
    assert out["found"] == 0 and out["flag_fail"] == 10
    with pytest.raises(pf.PFError):
        eng.p3p_histogram(blobs[:2])
    with pytest.raises(pf.PFError):
        eng.initialise(blobs, n_particles=10_000)  # > max_particles
    eng.close()


def test_initialise_keeps_resident_slot0():
    """Slot 0 is never written when K < N (the fill loop stops at PoseParticle[1], PE:1756)."""
    M, N = 5, 64
    eng = engine(M, N)
    prior = np.tile(syn.to12(syn.truth_pose(0.2)), (N, 1))
    eng.set_prior(prior)
    blobs, _ = syn.init_blobs(M, 2, 21)
    out, h = eng.initialise(blobs, n_particles=N)
    assert out["found"] == 1
    got = eng.get_particles(1)
    _, _, parts = orc.initialise(syn.markers_for(M), K, blobs, N, particles=prior, hist=h)
    np.testing.assert_allclose(got, parts, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(got[0], prior[0])
    eng.close()
