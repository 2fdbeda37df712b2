"""pfmpe_assoc_stats / pfmpe_get_pairs on the device: every particle's (LED, blob) pairs against the fp64 oracle's
likelihood on the rows the particle read-back returns, the votes table against the histogram of those rows, and the
identities that tie the two calls, the frame record and the host summary together.  Everything is integers: every
comparison is exact.

fp32 / fp16 state derives the pairs in fp32, so a particle may differ from the fp64 oracle where a decision sits on
a rounding: those particles ("fragile", margin tau = 1e-3 px, more than ten times the fp32 rounding of a projection
below 2,000 px) are set aside, at most 3 % of the set, and all others must agree exactly.  Observed on an MI355X
on the M=5 / B=50 / N=1000 input: fp32 state 1 / 1000 fragile particles in the propagated set and 0 in the
resampled set, fp16 state 2 and 5; no row differed from the oracle's, fragile or not."""
import ctypes
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from pf_monocular_pose_estimator_amd import _capi
from oracle import pforacle as orc
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = [pf.STATE_F64, pf.STATE_F32, pf.STATE_F16]
WHICH = [pf.ASSOC_PROPAGATED, pf.ASSOC_POSTERIOR]
TAU = 1e-3
MM = pf.MAX_MARKERS


markers_16 = syn.markers_16


@functools.lru_cache(maxsize=None)
def _stream(M, B, N, n_frames=1):
    return syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=N, heavy=(M == 12)), n_frames)


def _frame(eng, fr, f=0, blobs=None, **kw):
    return eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs if blobs is None else blobs,
                          dt=fr.dt, seed=900 + f, frame_idx=f, **kw)


def _stepped(M, B, N, state, fused=2):
    """An engine after one step of the (M, B, N) stream, with the frame's blobs and its record."""
    st = _stream(M, B, max(N, 1000))
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX, fused=fused)
    eng.set_prior(st.prior(fast=True)[:N])
    fr = st.frames[0]
    out = eng.step(_frame(eng, fr))
    return eng, st, st.markers, fr.blobs, out


def _hist(corr, n_corr, M, B):
    """votes (M, B + 1) and npairs_hist (M + 1) of pair rows."""
    N = len(n_corr)
    votes = np.zeros((M, B + 1), dtype=np.int64)
    live = np.arange(MM)[None, :] < n_corr[:, None]
    led, blob = corr[:, :, 0][live].astype(np.int64), corr[:, :, 1][live].astype(np.int64)
    assert np.all(corr[~live] == 0)
    if led.size:
        assert led.min() >= 1 and led.max() <= M and blob.min() >= 1 and blob.max() <= B
    np.add.at(votes, (led - 1, blob), 1)
    votes[:, 0] = N - votes[:, 1:].sum(axis=1)
    return votes, np.bincount(n_corr, minlength=M + 1)


def _oracle_rows(K, markers, poses, blobs, prm):
    """The oracle's pair rows of every pose, padded like the device rows, and the fragile flags."""
    N, M, B = len(poses), len(markers), len(blobs)
    corr = np.zeros((N, MM, 2), dtype=np.uint32)
    n_corr = np.zeros(N, dtype=np.int32)
    fragile = np.zeros(N, dtype=bool)
    for i, pose in enumerate(poses):
        proj = np.array([orc.project(K, pose, X) for X in markers])
        pairs = orc.likelihood(proj, blobs, prm.tol, prm.tol_pf)[1]
        n_corr[i] = len(pairs)
        corr[i, : len(pairs)] = pairs
        if B:
            d = np.sort(np.linalg.norm(blobs[:, None, :] - proj[None, :, :], axis=2), axis=0)  # (B, M), per LED
            near = d[0]
            fr = np.any(np.abs(near - prm.tol_pf) < TAU)
            if B > 1:
                fr |= np.any(d[1] - d[0] < TAU)
            ok = np.sort(near[near <= prm.tol_pf])
            fr |= np.any(np.diff(ok) < TAU)
            fragile[i] = fr
    return corr, n_corr, fragile


def _check_oracle(eng, st_K, mk, blobs, exact):
    prm = pf.default_params()
    M, B = len(mk), len(blobs)
    for which in WHICH:
        poses = eng.get_particles(which)
        N = len(poses)
        want_c, want_n, fragile = _oracle_rows(st_K, mk, poses, blobs, prm)
        got_c, got_n = eng.get_pairs(which, blobs=blobs)
        got = eng.assoc_stats(which, blobs=blobs)
        assert got_c.shape == (N, MM, 2) and got_n.shape == (N,)
        if exact:
            keep = np.ones(N, dtype=bool)
        else:
            keep = ~fragile
            print(f"which={which}: {int(fragile.sum())}/{N} fragile, "
                  f"{int(np.sum(np.any(got_c != want_c, axis=(1, 2)) | (got_n != want_n)))} rows differ")
            assert fragile.sum() <= 0.03 * N
        assert np.array_equal(got_n[keep], want_n[keep])
        assert np.array_equal(got_c[keep], want_c[keep])
        if exact:
            votes, hist = _hist(want_c, want_n, M, B)
            assert np.array_equal(got["votes"], votes)
            assert np.array_equal(got["npairs_hist"], hist)
            assert got["n"] == N and got["n_any"] == N - hist[0]


# ---- 1. oracle parity, fp64 state: exact
@pytest.mark.parametrize("M,B,N", [(5, 50, 1), (5, 50, 63), (5, 50, 64), (5, 50, 257), (5, 50, 1000),
                                   (4, 3, 1000), (12, 200, 1000)])
def test_oracle_parity_f64(M, B, N):
    """One lane, a partial wave, a full wave, a block plus one, a ragged tail; the min(B, M) cap; the 12-LED object."""
    eng, st, mk, blobs, _ = _stepped(M, B, N, pf.STATE_F64)
    try:
        _check_oracle(eng, st.K, mk, blobs, exact=True)
    finally:
        eng.close()


# ---- 2. oracle parity, fp32 compute: exact on the non-fragile particles
@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F16])
def test_oracle_parity_f32(state):
    eng, st, mk, blobs, _ = _stepped(5, 50, 1000, state)
    try:
        _check_oracle(eng, st.K, mk, blobs, exact=False)
    finally:
        eng.close()


# ---- 3. identities
def _check_identities(eng, blobs, out, M):
    B = len(blobs)
    N = eng.N
    for which in WHICH:
        corr, n_corr = eng.get_pairs(which, blobs=blobs, first=0, count=N)
        got = eng.assoc_stats(which, blobs=blobs)
        votes, hist = _hist(corr, n_corr, M, B)
        assert got["votes"].shape == (M, B + 1) and got["votes"].dtype == np.uint32
        assert np.array_equal(got["votes"], votes)
        assert np.array_equal(got["npairs_hist"], hist)
        assert got["n"] == N and (got["M"], got["B"]) == (M, B)
        assert np.all(got["votes"].astype(np.int64).sum(axis=1) == N)
        assert int(got["npairs_hist"].sum()) == N
        assert got["n_any"] == N - int(got["npairs_hist"][0])
        summ = pf.host_assoc_summary(got["votes"])
        for k, v in summ.items():
            assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    if out.resampled:
        assert np.array_equal(eng.get_particles(0)[out.winner_idx], np.array(out.winner_pose))
        c1, n1 = eng.get_pairs(pf.ASSOC_PROPAGATED, blobs=blobs, first=out.winner_idx, count=1)
        assert n1[0] == out.n_corr
        assert np.array_equal(c1[0, : n1[0]], out.pairs())


@pytest.mark.parametrize("state", STATES)
def test_identities(state):
    eng, st, mk, blobs, out = _stepped(5, 50, 1000, state)
    try:
        assert out.resampled
        _check_identities(eng, blobs, out, 5)
    finally:
        eng.close()


@pytest.mark.parametrize("state", STATES)
def test_identities_grid_stride_and_owner_gather(state):
    """N = 300,001: more particles than one grid of blocks, and a deferred prior read through its owner indices."""
    eng, st, mk, blobs, out = _stepped(5, 50, 300_001, state, fused=0)
    try:
        assert eng.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS
        assert out.resampled
        _check_identities(eng, blobs, out, 5)
    finally:
        eng.close()


# ---- 4. both voting paths
def test_direct_votes_large_table():
    """M = 16, B = 1024: the bins (64 KB) do not fit beside the blob table, every vote goes to the device table."""
    st = _stream(12, 200, 1000)
    fr = st.frames[0]
    mk = markers_16()
    rng = np.random.default_rng(3)
    true_px = syn.project(st.K, syn.to44(fr.current_pose), mk)  # the prior is centred on the frame's current pose
    near = true_px[rng.integers(0, 16, 400)] + rng.integers(1, 6, (400, 2)) * rng.choice([-1, 1], (400, 2))
    far = rng.uniform([0, 0], [syn.IMAGE_W, syn.IMAGE_H], size=(1024 - 16 - 400, 2))
    blobs = np.vstack([true_px, near, far])
    rng.shuffle(blobs)
    blobs = blobs.astype(np.float32).astype(np.float64)
    eng = pf.Engine(device=0, max_particles=1000, max_blobs=1024, state_dtype=pf.STATE_F32)
    try:
        eng.set_model(mk, st.K)
        eng.set_params(pf.default_params())
        eng.set_prior(st.prior(fast=True)[:1000])
        corr, n_corr = eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=blobs)
        got = eng.assoc_stats(pf.ASSOC_POSTERIOR, blobs=blobs)
        votes, hist = _hist(corr, n_corr, 16, 1024)
        print("n_any", got["n_any"], "npairs_hist", got["npairs_hist"].tolist())
        assert got["votes"].shape == (16, 1025)
        assert np.array_equal(got["votes"], votes) and np.array_equal(got["npairs_hist"], hist)
        assert got["n_any"] > 0  # the input does pair: the comparison is not of empty tables
    finally:
        eng.close()


@pytest.mark.parametrize("state", [pf.STATE_F64, pf.STATE_F32])
@pytest.mark.parametrize("M,B", [(5, 50), (12, 200)])
def test_lds_and_direct_votes_agree(M, B, state):
    """The LDS bins (the default at these sizes) and the direct path, pinned by the diagnostic switch, on one input:
    the same tables, and both equal the histogram of the pair rows."""
    eng, st, mk, blobs, _ = _stepped(M, B, 1000, state)
    try:
        for which in WHICH:
            corr, n_corr = eng.get_pairs(which, blobs=blobs)
            votes, hist = _hist(corr, n_corr, M, B)
            a = eng.assoc_stats(which, blobs=blobs)
            eng.set_option(pf.OPT_DIAG, pf.DIAG_ASSOC_DIRECT)
            b = eng.assoc_stats(which, blobs=blobs)
            eng.set_option(pf.OPT_DIAG, 0)
            assert np.array_equal(a["votes"], votes) and np.array_equal(a["npairs_hist"], hist)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    finally:
        eng.close()


# ---- 5. edge inputs
def test_edge_inputs():
    eng, st, mk, blobs, _ = _stepped(5, 50, 1000, pf.STATE_F32)
    N, M = 1000, 5
    try:
        for which in WHICH:
            none = eng.assoc_stats(which, blobs=np.zeros((0, 2)))
            assert none["votes"].shape == (M, 1) and np.all(none["votes"] == N)
            assert none["npairs_hist"][0] == N and none["n_any"] == 0 and none["B"] == 0
            c0, n0 = eng.get_pairs(which, blobs=np.zeros((0, 2)))
            assert not c0.any() and not n0.any()

            true_px = syn.project(st.K, st.frames[0].truth, mk)
            one = eng.assoc_stats(which, blobs=true_px[:1])
            c1, n1 = eng.get_pairs(which, blobs=true_px[:1])
            assert n1.max() == 1 and one["npairs_hist"][2:].sum() == 0 and one["n_any"] > 0
            assert np.array_equal(one["votes"], _hist(c1, n1, M, 1)[0])

            far = eng.assoc_stats(which, blobs=blobs + 1.0e5)
            assert far["votes"].shape == (M, 51) and np.all(far["votes"][:, 0] == N) and not far["votes"][:, 1:].any()
            assert far["npairs_hist"][0] == N and far["n_any"] == 0

            full_c, full_n = eng.get_pairs(which, blobs=blobs)
            part_c, part_n = eng.get_pairs(which, blobs=blobs, first=250, count=13)
            assert np.array_equal(part_c, full_c[250:263]) and np.array_equal(part_n, full_n[250:263])
            ec, en = eng.get_pairs(which, blobs=blobs, first=1000, count=0)
            assert ec.shape == (0, MM, 2) and en.shape == (0,)

        eng.stage_blob_bank([np.zeros((3, 2)), blobs])
        for which in WHICH:
            a = eng.assoc_stats(which, blobs=blobs)
            b = eng.assoc_stats(which, bank_frame=1)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
            ca, na = eng.get_pairs(which, blobs=blobs)
            cb, nb = eng.get_pairs(which, bank_frame=1)
            assert np.array_equal(ca, cb) and np.array_equal(na, nb)
    finally:
        eng.close()


# ---- 6. repeatable and side-effect free
def _raw_stats(eng, which, blobs):
    ai, keep = eng._assoc_in(blobs, -1)
    out = _capi.AssocOut()
    votes = np.zeros(eng.M * (len(blobs) + 1), dtype=np.uint32)
    rc = eng.lib.pfmpe_assoc_stats(eng.ctx, which, ctypes.byref(ai), ctypes.byref(out),
                                   votes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc == pf.OK
    return bytes(out) + votes.tobytes()


@pytest.mark.parametrize("fused", [2, 0])
def test_repeatable_and_side_effect_free(fused):
    N = 1000
    st = _stream(5, 50, N, 4)
    runs = []
    for with_assoc in (True, False):
        eng = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX, fused=fused)
        eng.set_prior(st.prior(fast=True))
        snaps = []
        try:
            for f, fr in enumerate(st.frames):
                out = eng.step(_frame(eng, fr, f))
                if with_assoc:
                    for which in WHICH:
                        assert _raw_stats(eng, which, fr.blobs) == _raw_stats(eng, which, fr.blobs)
                        a, b = eng.get_pairs(which, blobs=fr.blobs), eng.get_pairs(which, blobs=fr.blobs)
                        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                ref = np.array(out.winner_pose if out.resampled else out.most_likely_pose)
                s = {"out": out.as_dict(), "w": eng.get_weights(), "p0": eng.get_particles(0),
                     "p1": eng.get_particles(1)}
                for which in (pf.CLOUD_WEIGHTED, pf.CLOUD_POSTERIOR):
                    for k, v in eng.cloud_stats(which, ref=ref).items():
                        s[f"cloud{which}_{k}"] = np.asarray(v)
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


# ---- 7. after a batch
def test_after_step_multi():
    N = 1000
    st = _stream(5, 50, N, 2)
    priors = [st.prior(fast=True), st.prior(fast=True)[::-1].copy()]

    def fresh(s):
        e = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
        e.set_prior(priors[s])
        return e

    batch, twins = [fresh(0), fresh(1)], [fresh(0), fresh(1)]
    try:
        frames = [_frame(batch[s], st.frames[s], s) for s in range(2)]
        pf.Engine.step_multi(batch, frames)
        for s in range(2):
            twins[s].step(_frame(twins[s], st.frames[s], s))
            for which in WHICH:
                a = batch[s].assoc_stats(which, blobs=st.frames[s].blobs)
                b = twins[s].assoc_stats(which, blobs=st.frames[s].blobs)
                assert a["n_any"] > 0
                for k in a:
                    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (s, which, k)
    finally:
        for e in batch + twins:
            e.close()


# ---- 8. errors
def _code(fn, *a, **kw):
    with pytest.raises(pf.PFError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors():
    st = _stream(5, 50, 1000)
    fr = st.frames[0]
    blobs = fr.blobs
    eng = pf.Engine(device=0, max_particles=1000, max_blobs=64, state_dtype=pf.STATE_F32)
    try:
        assert _code(eng.assoc_stats, pf.ASSOC_POSTERIOR, blobs=blobs) == pf.E_STATE  # no model
        eng.set_model(st.markers, st.K)
        assert _code(eng.assoc_stats, pf.ASSOC_POSTERIOR, blobs=blobs) == pf.E_STATE  # no particle set
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, blobs=blobs, first=0, count=0) == pf.E_STATE
        eng.set_prior(st.prior(fast=True))
        assert _code(eng.assoc_stats, pf.ASSOC_PROPAGATED, blobs=blobs) == pf.E_STATE  # no step yet
        assert _code(eng.get_pairs, pf.ASSOC_PROPAGATED, blobs=blobs) == pf.E_STATE
        assert _code(eng.assoc_stats, 2, blobs=blobs) == pf.E_ARG
        assert _code(eng.get_pairs, -1, blobs=blobs) == pf.E_ARG
        assert _code(eng.assoc_stats, pf.ASSOC_POSTERIOR, bank_frame=0) == pf.E_ARG  # no bank staged
        eng.stage_blob_bank([blobs])
        assert _code(eng.assoc_stats, pf.ASSOC_POSTERIOR, bank_frame=1) == pf.E_ARG
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, bank_frame=7) == pf.E_ARG
        assert _code(eng.assoc_stats, pf.ASSOC_POSTERIOR, blobs=np.zeros((65, 2))) == pf.E_CAP
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, blobs=np.zeros((65, 2))) == pf.E_CAP
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, blobs=blobs, first=-1, count=1) == pf.E_ARG
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, blobs=blobs, first=0, count=-1) == pf.E_ARG
        assert _code(eng.get_pairs, pf.ASSOC_POSTERIOR, blobs=blobs, first=990, count=11) == pf.E_ARG

        lib, up, ip = eng.lib, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
        out = _capi.AssocOut()
        ai = _capi.AssocIn()
        ai.bank_frame = -1
        assert lib.pfmpe_assoc_stats(eng.ctx, 1, None, ctypes.byref(out), up()) == pf.E_ARG
        assert lib.pfmpe_assoc_stats(eng.ctx, 1, ctypes.byref(ai), None, up()) == pf.E_ARG
        ai.B = 4  # blobs NULL with B > 0
        assert lib.pfmpe_assoc_stats(eng.ctx, 1, ctypes.byref(ai), ctypes.byref(out), up()) == pf.E_ARG
        ai.B = -1
        assert lib.pfmpe_assoc_stats(eng.ctx, 1, ctypes.byref(ai), ctypes.byref(out), up()) == pf.E_ARG
        assert lib.pfmpe_get_pairs(eng.ctx, 1, ctypes.byref(ai), 0, 1, up(), ip()) == pf.E_ARG
        assert lib.pfmpe_assoc_stats(None, 1, ctypes.byref(ai), ctypes.byref(out), up()) == pf.E_ARG

        # and the context still works: a step, then both calls
        res = eng.step(_frame(eng, fr))
        got = eng.assoc_stats(pf.ASSOC_PROPAGATED, blobs=blobs, want_votes=False)
        assert got["n"] == 1000 and "votes" not in got and res.iters >= 1
        assert eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=blobs)[1].shape == (1000,)
    finally:
        eng.close()


# ---- 9. the single call's own codes and texts
def test_single_call_error_texts():
    """Every code and text of pfmpe_assoc_stats that an argument or a state can reach, in the order of its checks.  (A
    blob table that exceeds the LDS and an inconsistent votes table cannot be provoked through the API: the largest
    table max_blobs admits fits, and the bins are the kernel's own.)"""
    st = _stream(5, 50, 1000)
    blobs = st.frames[0].blobs
    eng = pf.Engine(device=0, max_particles=1000, max_blobs=64, state_dtype=pf.STATE_F32)
    lib, up, dp = eng.lib, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double)
    out = _capi.AssocOut()
    keep = np.ascontiguousarray(blobs, dtype=np.float64)

    def call(which=pf.ASSOC_POSTERIOR, B=50, ptr=True, bank_frame=-1, null_in=False, null_out=False):
        ai = _capi.AssocIn()
        ai.blobs = keep.ctypes.data_as(dp) if ptr else dp()
        ai.B = B
        ai.bank_frame = bank_frame
        rc = lib.pfmpe_assoc_stats(eng.ctx, which, None if null_in else ctypes.byref(ai),
                                   None if null_out else ctypes.byref(out), up())
        return rc, eng.last_error()

    try:
        # the argument checks come before the state checks: a context without a model reports them
        assert call(null_out=True) == (pf.E_ARG, "assoc_stats: null out")
        assert call(null_in=True) == (pf.E_ARG, "assoc_stats: bad arguments")
        assert call(which=2) == (pf.E_ARG, "assoc_stats: bad arguments")
        assert call(which=-1) == (pf.E_ARG, "assoc_stats: bad arguments")
        assert call(B=-1) == (pf.E_ARG, "assoc_stats: B < 0")
        assert call(bank_frame=0) == (pf.E_ARG, "assoc_stats: bank_frame out of range")
        assert call(B=4, ptr=False) == (pf.E_ARG, "assoc_stats: null blobs")
        assert call(B=65) == (pf.E_CAP, "assoc_stats: B exceeds max_blobs")
        assert call() == (pf.E_STATE, "assoc_stats: set_model and a particle set first")
        eng.set_model(st.markers, st.K)
        assert call() == (pf.E_STATE, "assoc_stats: set_model and a particle set first")
        eng.set_prior(st.prior(fast=True))
        assert call(which=pf.ASSOC_PROPAGATED) == (pf.E_STATE, "assoc_stats(propagated): no step yet")
        eng.stage_blob_bank([blobs])
        assert call(bank_frame=1) == (pf.E_ARG, "assoc_stats: bank_frame out of range")
        assert call()[0] == pf.OK and call(bank_frame=0)[0] == pf.OK and out.B == 50
    finally:
        eng.close()


# ---- 10. the single call and the batch on one context's scratch
def _same_stats(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def test_single_call_shares_scratch_with_batches():
    """A batch of three B = 50 entries, a single call with B = 1, a single call with B = 50 on a context that has only
    ever run B = 1, a batch again: every record and table equals that of a context that ran nothing else."""
    made = [_stepped(5, 50, 1000, pf.STATE_F32) for _ in range(4)]
    a, c, fresh50, fresh1 = [m[0] for m in made]
    blobs = made[0][3]
    try:
        ref50 = {w: fresh50.assoc_stats(w, blobs=blobs) for w in WHICH}
        ref1 = {w: fresh1.assoc_stats(w, blobs=blobs[:1]) for w in WHICH}
        assert all(ref50[w]["n_any"] > 0 for w in WHICH)
        whichs = [pf.ASSOC_PROPAGATED, pf.ASSOC_POSTERIOR, pf.ASSOC_PROPAGATED]
        for s, got in enumerate(pf.Engine.assoc_stats_multi([a] * 3, whichs, [blobs] * 3)):
            _same_stats(got, ref50[whichs[s]], ("first batch", s))
        for w in WHICH:
            _same_stats(a.assoc_stats(w, blobs=blobs[:1]), ref1[w], ("single B=1 after a batch", w))
        for w in WHICH:
            _same_stats(c.assoc_stats(w, blobs=blobs[:1]), ref1[w], ("single B=1", w))
        for w in WHICH:
            _same_stats(c.assoc_stats(w, blobs=blobs), ref50[w], ("single B=50 after B=1", w))
        for s, got in enumerate(pf.Engine.assoc_stats_multi([a, c, a], whichs, [blobs] * 3)):
            _same_stats(got, ref50[whichs[s]], ("second batch", s))
    finally:
        for e in (a, c, fresh50, fresh1):
            e.close()


# ---- 11. what the single call adds to the kernel statistics
# read once on the build whose single call had a path of its own: launches per kernel name added by one call.  Neither
# adds any: the association launches are not bracketed, the step's own brackets are harvested by the statistics read
# before the call, and a PROPAGATED call's regeneration opens its aux bracket only inside a sampled frame.
SINGLE_CALL_ADDS = {pf.ASSOC_POSTERIOR: {}, pf.ASSOC_PROPAGATED: {}}


def test_single_call_kernel_stats():
    """With every frame sampled (OPT_TIMING 1): the launches a POSTERIOR and a PROPAGATED single call add to
    pfmpe_get_kernel_stats (the kernels not named in SINGLE_CALL_ADDS: none)."""
    st = _stream(5, 50, 1000)
    eng = make_engine(1000, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
    try:
        eng.set_option(pf.OPT_TIMING, 1)
        eng.set_prior(st.prior(fast=True))
        fr = st.frames[0]
        eng.step(_frame(eng, fr))
        for which in (pf.ASSOC_POSTERIOR, pf.ASSOC_PROPAGATED):
            before = eng.kernel_stats()
            eng.assoc_stats(which, blobs=fr.blobs)
            after = eng.kernel_stats()
            added = {k: after[k][0] - before[k][0] for k in after if after[k][0] != before[k][0]}
            print("which", which, "adds", added)
            assert added == SINGLE_CALL_ADDS[which]
    finally:
        eng.close()


# ---- 12. the single call against a batch entry without blobs
@pytest.mark.parametrize("N", [1, 257])
def test_single_equals_batch_entry_without_blobs(N):
    eng, st, mk, blobs, _ = _stepped(5, 50, N, pf.STATE_F32)
    none = np.zeros((0, 2))
    try:
        for which in WHICH:
            want = _raw_stats(eng, which, none)
            ai, keep = eng._assoc_in(none, -1)
            ins = (_capi.AssocMultiIn * 1)()
            ins[0].blobs = ai
            ins[0].which = which
            outs = (_capi.AssocOut * 1)()
            votes = np.zeros(eng.M, dtype=np.uint32)
            vps = (ctypes.POINTER(ctypes.c_uint32) * 1)(votes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
            ctxs = (ctypes.c_void_p * 1)(eng.ctx.value)
            assert eng.lib.pfmpe_assoc_stats_multi(ctxs, 1, ins, outs, vps) == pf.OK
            assert bytes(outs[0]) + votes.tobytes() == want
            assert outs[0].n == N and outs[0].n_any == 0 and np.all(votes == N)
    finally:
        eng.close()
