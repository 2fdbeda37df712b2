"""The flat one-launch frame's tail (k_frame2: DESIGN.md §4.0b, round 7) against the two-launch frame, byte for byte.

k_frame2 publishes each block's count partial and winner candidate before the block's scatter, evaluates K_total
in the count phase instead of the top, and forms the block's weight prefix while it waits at the weighing barrier.
None of that changes a rounding, an association or an RNG draw, so every output must equal the two-launch run's
(PFMPE_OPT_FUSED = 0, whose resampling code is separate): every record field, the new prior, the kept propagated
set, the weights and the resample counts.  The tree one-launch frame (PFMPE_OPT_FUSED = 1) is compared as well; it
may run as two launches where its residency rule says so, so its shape is not asserted.
"""
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc
from test_gpu_parity import RNG, STATE, make_engine

pytestmark = pytest.mark.gpu


def _snapshot(eng, out):
    snap = {"out": out, "w": eng.get_weights(), "p0": eng.get_particles(0), "p1": eng.get_particles(1)}
    if out["resampled"]:
        snap["counts"] = eng.get_counts()
    return snap


def _run(st, N, state, rng, fused, frames, prior=None, diag=0):
    """frames: a list of make_frame keyword dicts.  Returns one snapshot per frame."""
    eng = make_engine(N, st.markers, st.K, state, rng, fused=fused)
    if diag:
        eng.set_option(pf.OPT_DIAG, diag)
    eng.set_prior(st.prior() if prior is None else prior)
    snaps = []
    for kw in frames:
        out = eng.step(eng.make_frame(**kw)).as_dict()
        if fused == 2:
            assert eng.info(pf.INFO_LAST_SHAPE) == pf.SHAPE_FRAME2
        elif fused == 0:
            assert eng.info(pf.INFO_LAST_SHAPE) == pf.SHAPE_TWO_LAUNCH
        snaps.append(_snapshot(eng, out))
    if fused == 2:
        assert eng.info(pf.INFO_FUSED_FALLBACKS) == 0
    eng.close()
    return snaps


def _assert_same(a, b, tag):
    assert len(a) == len(b)
    for f, (x, y) in enumerate(zip(a, b)):
        for k, v in x["out"].items():
            assert np.array_equal(np.asarray(v), np.asarray(y["out"][k])), (tag, f, k)
        for k in ("p1", "p0", "w", "counts"):
            assert (k in x) == (k in y), (tag, f, k)
            if k in x:
                assert x[k].tobytes() == y[k].tobytes(), (tag, f, k)


def _frame_kw(fr, seed, blobs=None, **kw):
    return dict(current_pose=fr.current_pose, predicted_pose=fr.predicted_pose, prediction=fr.prediction,
                blobs=fr.blobs if blobs is None else blobs, dt=fr.dt, seed=seed, frame_idx=fr.index, **kw)


@pytest.mark.parametrize("rng", ["philox", "ref"])
@pytest.mark.parametrize("state", ["f32", "f64"])
@pytest.mark.parametrize("N", [257, 1000, 4161])
def test_ragged_sizes(N, state, rng):
    """N = 257: the second block has one valid lane and three waves without any; 1,000 and 4,161: a ragged last
    block after several full ones.  fp32 state takes the integer wave scan, fp64 the fp64 scan.  Three steady
    frames, each starting from the prior the frame before scattered."""
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=30, N=N), 3)
    frames = [_frame_kw(fr, 40 + fr.index) for fr in st.frames]
    base = _run(st, N, STATE[state], RNG[rng], 0, frames)
    assert any(s["out"]["resampled"] for s in base)
    for fused in (2, 1):
        _assert_same(_run(st, N, STATE[state], RNG[rng], fused, frames), base, f"fused={fused}")


def _occluded_blobs(st, fr, B, seed):
    true_px = syn.project(st.K, fr.truth, st.markers)
    outl = np.random.default_rng(seed).uniform([0, 0], [syn.IMAGE_W, syn.IMAGE_H], size=(B - len(true_px) + 1, 2))
    return np.vstack([true_px[1:], outl]).astype(np.float32).astype(np.float64)


_OCC_B, _OCC_ITERS = 30, 12


@functools.lru_cache(maxsize=None)
def _early_kept_seed():
    """A frame seed for which the oracle (fp64, Philox, N = 1,000, one LED occluded, 12 forced iterations) keeps an
    iteration earlier than the last on at least one of the two frames."""
    N = 1000
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=_OCC_B, N=N), 2)
    for seed in range(13, 33):
        prior = st.prior()
        early = False
        for fr in st.frames:
            ref, arr = orc.pf_step(st.markers, st.K, orc.make_params(rng_mode=pf.RNG_PHILOX), prior, fr.current_pose,
                                   fr.predicted_pose, fr.prediction, _occluded_blobs(st, fr, _OCC_B, fr.index),
                                   dt=fr.dt, seed=seed, frame_idx=fr.index, force_iters=_OCC_ITERS)
            early |= ref["kept_iter"] < ref["iters"] - 1
            if ref["resampled"]:
                prior = arr["resampled"]
        if early:
            return seed
    raise AssertionError("no seed keeps an earlier iteration")


@pytest.mark.parametrize("state", ["f32", "f64"])
@pytest.mark.parametrize("N", [1000, 20_000])
def test_kept_iteration_earlier_than_the_last(N, state):
    """One LED occluded and 12 forced iterations: the kept iteration is an earlier one, so the weights in registers
    at the end of the loop are not the kept ones and the prefix formed at the last barrier must be discarded (the
    phase recomputes it from the re-read weights).  Also with a lagging reader (DIAG_LAG_LOADS) and with the min-side
    scans forced (DIAG_MIN_SIDE)."""
    seed = _early_kept_seed()
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=_OCC_B, N=N), 2)
    frames = [_frame_kw(fr, seed, blobs=_occluded_blobs(st, fr, _OCC_B, fr.index), force_iters=_OCC_ITERS)
              for fr in st.frames]
    base = _run(st, N, STATE[state], pf.RNG_PHILOX, 0, frames)
    for s in base:
        assert s["out"]["iters"] == _OCC_ITERS
    assert any(s["out"]["kept_iter"] < s["out"]["iters"] - 1 and s["out"]["resampled"] for s in base)
    for fused, diag in ((2, 0), (2, pf.DIAG_LAG_LOADS), (2, pf.DIAG_MIN_SIDE), (1, 0)):
        _assert_same(_run(st, N, STATE[state], pf.RNG_PHILOX, fused, frames, diag=diag), base,
                     f"fused={fused} diag={diag}")


def _far(pose12):
    """The pose moved 1 m sideways: none of its LEDs projects near its blob."""
    p = np.array(pose12, dtype=np.float64).reshape(12).copy()
    p[3] += 1.0
    return p


@pytest.mark.parametrize("state", ["f32", "f64"])
@pytest.mark.parametrize("where", ["wave1_middle_block", "wave0_block0", "last_lane_last_block"])
def test_one_particle_takes_nearly_every_copy(where, state):
    """Only one particle of the prior is well placed (the frame's current and predicted poses, which the motion
    model puts at indices 0 and 1, are far off too), so its write range spans many 64-slot chunks of the scatter,
    K_total is exercised and most blocks have no copies (their candidate is regenerated).  The particle sits in
    wave 1 of a middle block (the wave that publishes the candidate before it scatters), in wave 0 of block 0 (the
    wave that writes the record before it scatters) or in the last valid lane of the last block."""
    N = 3000
    idx = {"wave1_middle_block": 256 * 5 + 64 + 3, "wave0_block0": 5, "last_lane_last_block": N - 1}[where]
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=20, N=N), 1)
    fr = st.frames[0]
    good = syn.to12(fr.truth)
    prior = np.tile(_far(good), (N, 1))
    prior[idx] = good
    ident = np.eye(4)[:3].reshape(12)
    frames = [dict(current_pose=_far(good), predicted_pose=_far(good), prediction=ident, blobs=fr.blobs, dt=fr.dt,
                   seed=61, frame_idx=0)]
    base = _run(st, N, STATE[state], pf.RNG_PHILOX, 0, frames, prior=prior)
    out = base[0]["out"]
    assert out["accepted"] == 1 and out["resampled"] == 1
    assert out["winner_idx"] == idx
    counts = base[0]["counts"].astype(np.int64)
    assert counts.sum() == N
    assert counts[idx] > 0.9 * N
    for fused in (2, 1):
        got = _run(st, N, STATE[state], pf.RNG_PHILOX, fused, frames, prior=prior)
        _assert_same(got, base, f"fused={fused}")
        assert got[0]["out"]["winner_idx"] == idx
        assert np.array_equal(got[0]["out"]["pairs"], out["pairs"])
        assert int(got[0]["counts"].astype(np.int64).sum()) == N


@pytest.mark.parametrize("state", ["f32", "f64"])
def test_frames_without_resampling(state):
    """A frame without blobs and a frame whose blobs are all far away are not accepted (no resampling: block 0
    writes the record alone); the normal frame after them on the same engine resamples as usual."""
    N = 3000
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=30, N=N), 3)
    f0, f1, f2 = st.frames
    frames = [_frame_kw(f0, 9, blobs=np.zeros((0, 2))),
              _frame_kw(f1, 10, blobs=np.array([[5000.0, 5000.0], [6000.0, -40.0]]), force_iters=4),
              _frame_kw(f2, 11)]
    base = _run(st, N, STATE[state], pf.RNG_PHILOX, 0, frames)
    assert [s["out"]["accepted"] for s in base] == [0, 0, 1]
    assert base[2]["out"]["resampled"] == 1
    for fused in (2, 1):
        _assert_same(_run(st, N, STATE[state], pf.RNG_PHILOX, fused, frames), base, f"fused={fused}")


def test_closed_loop_of_30_frames():
    """30 consecutive frames through step_batch: each frame's prior is the complete scatter of the frame before
    (which now ends after that frame's record is published), read back right after the last step."""
    N, F = 3000, 30
    st = syn.make_stream(syn.StreamConfig("t", M=5, B=30, N=N), F)
    res = {}
    for fused in (0, 2, 1):
        eng = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX, fused=fused)
        eng.set_prior(st.prior())
        eng.stage_blob_bank([f.blobs for f in st.frames])
        frames = [eng.make_frame(f.current_pose, f.predicted_pose, f.prediction, B=len(f.blobs), bank_frame=f.index,
                                 dt=f.dt, seed=70 + f.index, frame_idx=f.index) for f in st.frames]
        recs = [o.as_dict() for o in eng.step_batch(frames)]
        post = eng.get_particles(1)
        if fused == 2:
            assert eng.info(pf.INFO_LAST_SHAPE) == pf.SHAPE_FRAME2
            assert eng.info(pf.INFO_FUSED_FALLBACKS) == 0
        res[fused] = (recs, post, eng.get_particles(0), eng.get_weights(), eng.get_counts())
        eng.close()
    assert sum(r["resampled"] for r in res[0][0]) >= F - 2
    for fused in (2, 1):
        for f, (a, b) in enumerate(zip(res[fused][0], res[0][0])):
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (fused, f, k)
        for x, y in zip(res[fused][1:], res[0][1:]):
            assert x.tobytes() == y.tobytes(), fused
