"""pfmpe_cloud_stats on the device against the numpy restatement of its definition (tests/cloud_ref.py) evaluated on
the rows and weights the read-backs return.

Tolerance, every array: |got - want| <= 1e-9 * max|want| (cov: 1e-9 * its largest diagonal entry).  Both sides are
fp64 on identical inputs with the same operations per particle, so they differ by libm rounding and by the order of
the sums over particles: at most N * 2^-53 ~ 3e-11 of the absolute sum at N = 3e5, times ~3.5 for the cancellation
in C = E[xi xi^T] - mu mu^T on these priors (mean twist ~1.6 sigma)."""
import ctypes
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from pf_monocular_pose_estimator_amd import _capi
from test_gpu_parity import make_engine
from test_gpu_defer import _frames

import cloud_ref

pytestmark = pytest.mark.gpu

STATES = [pf.STATE_F64, pf.STATE_F32, pf.STATE_F16]


@functools.lru_cache(maxsize=None)
def _stream(N, n_frames):
    return syn.make_stream(syn.StreamConfig("t", M=5, B=50, N=N), n_frames)


def _frame(eng, fr, f, blobs=None, **kw):
    return eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs if blobs is None else blobs,
                          dt=fr.dt, seed=900 + f, frame_idx=f, **kw)


def _default_ref(out):
    return np.array(out.winner_pose if out.resampled else out.most_likely_pose)


def _check_both(eng, out):
    """WEIGHTED and POSTERIOR with the default reference against numpy on the read-backs."""
    ref = _default_ref(out)
    w = eng.get_weights()
    got = eng.cloud_stats(pf.CLOUD_WEIGHTED)
    cloud_ref.check(got, cloud_ref.stats(eng.get_particles(0), w, ref))
    assert abs(got["wsum"] - out.prob_sum) <= 1e-9 * out.prob_sum
    cloud_ref.check(eng.cloud_stats(pf.CLOUD_POSTERIOR), cloud_ref.stats(eng.get_particles(1), None, ref))


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N", [1, 63, 64, 257, 1000])
def test_prior_only(N, state):
    """One lane, a partial wave, a full wave, a block plus one particle, a block tail that is no multiple of 64."""
    st = _stream(1000, 1)
    prior = st.prior(fast=True)[:N]
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX)
    try:
        eng.set_prior(prior)
        with pytest.raises(ValueError):
            eng.cloud_stats(pf.CLOUD_POSTERIOR)  # no step yet: the reference must be given
        got = eng.cloud_stats(pf.CLOUD_POSTERIOR, ref=prior[0])
        want = cloud_ref.stats(eng.get_particles(1), None, prior[0])
    finally:
        eng.close()
    assert got["n"] == N and got["ess"] == N and got["wsum"] == N and got["degenerate"] == 0
    cloud_ref.check(got, want)
    if N == 1:
        assert np.array_equal(got["cov"], np.zeros((6, 6)))


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N", [1000, 4097])
def test_after_two_steps(N, state):
    st = _stream(N, 2)
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX)
    try:
        eng.set_prior(st.prior(fast=True))
        for f, fr in enumerate(st.frames):
            out = eng.step(_frame(eng, fr, f))
        assert out.resampled
        _check_both(eng, out)
    finally:
        eng.close()


@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F16])
def test_grid_stride_and_owner_gather(state):
    """N = 300,001: 1172 blocks of particles on the 1024-block grid, and a deferred prior read through its owner
    indices."""
    N = 300_001
    st = _stream(N, 1)
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX, fused=0)
    try:
        eng.set_prior(st.prior(fast=True))
        out = eng.step(_frame(eng, st.frames[0], 0))
        assert eng.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS
        _check_both(eng, out)
    finally:
        eng.close()


@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F16])
def test_deferred_equals_materialised(state):
    """The shape sequence of test_gpu_defer (two-launch deferred, k_frame2, deferred, k_frame, deferred, regenerating):
    the statistics of both kinds are the same bits with deferral on and off, frame after frame."""
    N = 120_017
    st = _stream(N, 6)
    frames = _frames(st)
    shapes = [(0, 1), (2, 1), (0, 1), (1, 1), (0, 1), (0, 0)]  # (PFMPE_OPT_FUSED, keep propagated)
    runs = []
    for defer in (1, 0):
        eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX)
        eng.set_option(pf.OPT_DEFER_RESAMPLE, defer)
        eng.set_prior(st.prior(fast=True))
        snaps = []
        try:
            for f, ((fr, blobs, kw), (fused, keep)) in enumerate(zip(frames, shapes)):
                eng.set_option(pf.OPT_FUSED, fused)
                eng.set_option(pf.OPT_KEEP_PROPAGATED, keep)
                eng.step(_frame(eng, fr, f, blobs=blobs, **kw))
                snaps.append((eng.cloud_stats(pf.CLOUD_WEIGHTED), eng.cloud_stats(pf.CLOUD_POSTERIOR)))
        finally:
            eng.close()
        runs.append(snaps)
    for f, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (f, k)


def _raw(eng, which, ref):
    out = _capi.CloudOut()
    r = np.ascontiguousarray(ref, dtype=np.float64)
    rc = eng.lib.pfmpe_cloud_stats(eng.ctx, which, r.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(out))
    assert rc == pf.OK
    return bytes(out)


@pytest.mark.parametrize("fused,state", [(2, pf.STATE_F32), (0, pf.STATE_F32), (0, pf.STATE_F16)])
def test_repeatable_and_side_effect_free(fused, state):
    """Two calls return the same bytes; a 4-frame run with both statistics taken after every frame equals the run
    without them in every frame record, particle set, weight and count."""
    N = 120_017
    st = _stream(N, 6)
    runs = []
    for with_stats in (True, False):
        eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX, fused=fused)
        eng.set_prior(st.prior(fast=True))
        snaps = []
        try:
            for f, fr in enumerate(st.frames[:4]):
                out = eng.step(_frame(eng, fr, f))
                if with_stats:
                    ref = _default_ref(out)
                    for which in (pf.CLOUD_WEIGHTED, pf.CLOUD_POSTERIOR):
                        assert _raw(eng, which, ref) == _raw(eng, which, ref)
                s = {"out": out.as_dict(), "w": eng.get_weights(), "p0": eng.get_particles(0),
                     "p1": eng.get_particles(1)}
                if out.resampled:
                    s["counts"] = eng.get_counts()
                snaps.append(s)
        finally:
            eng.close()
        runs.append(snaps)
    for f, (x, y) in enumerate(zip(*runs)):
        assert x.keys() == y.keys(), f
        for k, v in x["out"].items():
            assert np.array_equal(np.asarray(v), np.asarray(y["out"][k])), (f, k)
        for k in x:
            if k != "out":
                assert np.array_equal(x[k], y[k]), (f, k)


def test_degenerate_weights():
    """A frame without blobs takes the re-initialisation branch with every weight zero."""
    N = 1000
    st = _stream(N, 2)
    eng = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
    try:
        eng.set_prior(st.prior(fast=True))
        out = eng.step(_frame(eng, st.frames[0], 0, blobs=np.zeros((0, 2))))
        assert out.prob_sum == 0 and not out.resampled
        got = eng.cloud_stats(pf.CLOUD_WEIGHTED)
    finally:
        eng.close()
    assert got["degenerate"] == 1 and got["n"] == N and got["wsum"] == 0 and got["ess"] == 0
    assert np.array_equal(got["mean_twist"], np.zeros(6)) and np.array_equal(got["cov"], np.zeros((6, 6)))
    assert np.array_equal(got["mean_pose"], np.array(out.most_likely_pose))
    assert got["max_trans"] == 0 and got["max_rot"] == 0


def test_errors():
    st = _stream(1000, 2)
    prior = st.prior(fast=True)
    eng = make_engine(1000, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
    try:
        with pytest.raises(pf.PFError) as e:
            eng.cloud_stats(pf.CLOUD_POSTERIOR, ref=prior[0])
        assert e.value.code == pf.E_STATE  # no particle set
        eng.set_prior(prior)
        with pytest.raises(pf.PFError) as e:
            eng.cloud_stats(pf.CLOUD_WEIGHTED, ref=prior[0])
        assert e.value.code == pf.E_STATE  # no step yet
        with pytest.raises(pf.PFError) as e:
            eng.cloud_stats(2, ref=prior[0])
        assert e.value.code == pf.E_ARG
        bad = prior[0].reshape(12).copy()
        bad[7] = np.nan
        with pytest.raises(pf.PFError) as e:
            eng.cloud_stats(pf.CLOUD_POSTERIOR, ref=bad)
        assert e.value.code == pf.E_ARG
        r = np.ascontiguousarray(prior[0])
        dp = ctypes.POINTER(ctypes.c_double)
        assert eng.lib.pfmpe_cloud_stats(eng.ctx, pf.CLOUD_POSTERIOR, r.ctypes.data_as(dp), None) == pf.E_ARG
        assert eng.lib.pfmpe_cloud_stats(eng.ctx, pf.CLOUD_POSTERIOR, dp(), ctypes.byref(_capi.CloudOut())) == pf.E_ARG
        assert eng.cloud_stats(pf.CLOUD_POSTERIOR, ref=prior[0])["n"] == 1000  # and the context still works
    finally:
        eng.close()


def test_error_texts():
    """Every validation failure of the single call returns its code and its exact last-error text (the strings are
    copied from the source of the version whose single call had a host path of its own), in the order of the checks:
    arguments, reference pose, particle set, kept set.  The output record is untouched, and after each failure the
    context steps and both of its statistics agree with numpy."""
    N = 1000
    st = _stream(N, 7)
    prior = st.prior(fast=True)
    good = np.ascontiguousarray(prior[0], dtype=np.float64).reshape(12)
    nan_ref, inf_ref = good.copy(), good.copy()
    nan_ref[7] = np.nan
    inf_ref[0] = -np.inf
    dp = ctypes.POINTER(ctypes.c_double)
    W, P = pf.CLOUD_WEIGHTED, pf.CLOUD_POSTERIOR
    ARGS, REF = "cloud_stats: bad arguments", "cloud_stats: non-finite reference pose"
    NO_SET, NO_STEP = "cloud_stats: no particle set", "cloud_stats(weighted): no step yet"

    def fails(eng, which, ref, code, text, null_out=False):
        out = _capi.CloudOut()
        ctypes.memset(ctypes.byref(out), 0xA5, ctypes.sizeof(out))
        rc = eng.lib.pfmpe_cloud_stats(eng.ctx, which, dp() if ref is None else ref.ctypes.data_as(dp),
                                       None if null_out else ctypes.byref(out))
        assert (rc, eng.last_error()) == (code, text)
        assert bytes(out) == b"\xa5" * ctypes.sizeof(out)

    def works(eng, f):
        _check_both(eng, eng.step(_frame(eng, st.frames[f], f)))

    # a context without particles: the argument checks come first, then the reference pose, then the state
    for which, ref, code, text in ((P, None, pf.E_ARG, ARGS), (3, good, pf.E_ARG, ARGS), (P, nan_ref, pf.E_ARG, REF),
                                   (P, good, pf.E_STATE, NO_SET), (W, good, pf.E_STATE, NO_SET)):
        eng = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
        try:
            fails(eng, which, ref, code, text)
            eng.set_prior(prior)
            works(eng, 0)
        finally:
            eng.close()
    eng = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
    try:
        assert eng.lib.pfmpe_cloud_stats(None, P, good.ctypes.data_as(dp), ctypes.byref(_capi.CloudOut())) == pf.E_ARG
        eng.set_prior(prior)
        fails(eng, W, good, pf.E_STATE, NO_STEP)
        works(eng, 0)
        cases = [(P, None, pf.E_ARG, ARGS, False), (W, good, pf.E_ARG, ARGS, True), (2, good, pf.E_ARG, ARGS, False),
                 (-1, good, pf.E_ARG, ARGS, False), (W, nan_ref, pf.E_ARG, REF, False),
                 (P, inf_ref, pf.E_ARG, REF, False)]
        for f, (which, ref, code, text, null_out) in enumerate(cases, start=1):
            fails(eng, which, ref, code, text, null_out)
            works(eng, f)
    finally:
        eng.close()
