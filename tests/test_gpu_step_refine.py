"""pfmpe_step_refine / pfmpe_step_refine_multi on the device: the step and the refinement of its winner in one call.

The calls are defined by equivalence, so every case runs twin engines (same model, prior, frames, Philox stream): one
makes the two existing calls (step, then refine_poses of the winner; step_multi, then refine_multi), the other the
fused call.  Everything is compared as bytes (the frame record, the summary, the row, the covariance, the posterior
set after the last frame): the tail runs the function k_refine runs on the numbers the two-call sequence sends back
up, so no tolerance is involved.  pfmpe_host_step_tail is the same code on the host and must give the same bytes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

pytestmark = pytest.mark.gpu

INT_KEYS = ("n", "n_with_pairs", "n_converged", "n_cap_kept", "n_cap_reverted", "iters_total", "iters_max", "best")
STATES = {"f64": pf.STATE_F64, "f32": pf.STATE_F32, "f16": pf.STATE_F16}
# name -> (PFMPE_OPT_FUSED, PFMPE_OPT_DEFER_RESAMPLE, the shape, the two-launch resampling launch)
SHAPES = {"frame2": (2, 1, pf.SHAPE_FRAME2, None), "frame": (1, 1, pf.SHAPE_FRAME, None),
          "owners": (0, 1, pf.SHAPE_TWO_LAUNCH, pf.RESAMPLE_OWNERS), "blocks": (0, 0, pf.SHAPE_TWO_LAUNCH, pf.RESAMPLE_BLOCKS)}
ROW_FILL, COV_FILL = 0x5A, -7.25


@functools.lru_cache(maxsize=None)
def stream(M=5, B=20, n_frames=4, seed=0):
    return syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=0, seed=seed), n_frames)


@functools.lru_cache(maxsize=None)
def prior_of(M, B, seed, N):
    p = stream(M, B, 4, seed).prior(N)
    p.setflags(write=False)
    return p


def engine(N, st, state=pf.STATE_F32, fused=2, defer=1, seed=0):
    e = pf.Engine(device=0, max_particles=N, state_dtype=state)
    e.set_option(pf.OPT_FUSED, fused)
    e.set_option(pf.OPT_DEFER_RESAMPLE, defer)
    e.set_model(st.markers, st.K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_PHILOX
    e.set_params(prm)
    e.set_prior(prior_of(st.cfg.M, st.cfg.B, seed, N))
    return e


def frame_in(e, fr, blobs=None, bank_frame=-1, force_iters=0, seed=77):
    if bank_frame >= 0:
        return e.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, B=len(fr.blobs), dt=fr.dt, seed=seed,
                            frame_idx=fr.index, force_iters=force_iters, bank_frame=bank_frame)
    blobs = fr.blobs if blobs is None else blobs
    return e.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=blobs, B=0, dt=fr.dt, seed=seed,
                        frame_idx=fr.index, force_iters=force_iters)


def buffers():
    row = pf.RefineRow.from_buffer_copy(bytes([ROW_FILL]) * C.sizeof(pf.RefineRow))
    return row, np.full(36, COV_FILL)


def refined(out):
    return out.flag_fail == pf.FLAG_ACCEPTED and bool(np.isfinite(np.array(out.winner_pose)).all())


def two_call(e, fi, params=None):
    """step, then refine_poses of the winner (K = 1) or of nothing (K = 0): (frame bytes, summary bytes, row bytes,
    cov bytes, FrameOut)."""
    out = e.step(fi)
    ai = pf.AssocIn(fi.blobs, fi.B, fi.bank_frame)
    gn = pf.RefineOut()
    row, cov = buffers()
    e._chk(e.lib.pfmpe_refine_poses(e.ctx, C.byref(ai), C.byref(params) if params is not None else None,
                                    out.winner_pose, out.corr, 1 if refined(out) else 0, C.byref(gn),
                                    C.addressof(row), cov.ctypes.data_as(C.POINTER(C.c_double))))
    return bytes(out), bytes(gn), bytes(row), cov.tobytes(), out


def fused_call(e, fi, params=None):
    row, cov = buffers()
    out, gn, row, cov = e.step_refine(fi, params=params, row=row, cov=cov)
    return bytes(out), bytes(gn), bytes(row), cov.tobytes(), out


def untouched(res):
    return res[2] == bytes([ROW_FILL]) * C.sizeof(pf.RefineRow) and res[3] == np.full(36, COV_FILL).tobytes()


def assert_same(a, b, tag):
    for k, name in enumerate(("frame_out", "summary", "row", "cov")):
        assert a[k] == b[k], (tag, name)


def empty_summary(gn_bytes):
    gn = pf.RefineOut.from_buffer_copy(gn_bytes)
    zeros = not np.frombuffer(bytes(gn.best_row), dtype=np.uint8).any() and not np.array(gn.best_cov).any()
    return gn.n == 0 and gn.best == -1 and zeros and all(getattr(gn, k) == 0 for k in INT_KEYS[1:-1])


def host_tail(st, blobs, res, params=None):
    row, cov = buffers()
    gn, row, cov = pf.host_step_tail(st.markers, st.K, blobs, res[4], params=params, row=row, cov=cov)
    return bytes(gn), bytes(row), cov.tobytes()


# ------------------------------------------------------------------------------- cases 1, 2, 8: shapes, types, buckets
@functools.lru_cache(maxsize=None)
def run_twins(shape, state, M=5, B=20, N=700):
    """Four frames on twins in one frame shape: the two-call results, the fused results, the shape each engine reports,
    the fused engine's fallback count and both posterior sets."""
    fused, defer, _, _ = SHAPES[shape]
    st = stream(M, B)
    a, b = engine(N, st, STATES[state], fused, defer), engine(N, st, STATES[state], fused, defer)
    try:
        ra, rb, shapes = [], [], []
        for fr in st.frames:
            ra.append(two_call(a, frame_in(a, fr)))
            rb.append(fused_call(b, frame_in(b, fr)))
            shapes.append((a.info(pf.INFO_LAST_SHAPE), b.info(pf.INFO_LAST_SHAPE), b.info(pf.INFO_LAST_RESAMPLE)))
        return ra, rb, shapes, b.info(pf.INFO_TAIL_FALLBACKS), a.get_particles(1).tobytes(), b.get_particles(1).tobytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_frame_shape_every_state_type(shape, state):
    ra, rb, shapes, fallbacks, pa, pb = run_twins(shape, state)
    _, _, want_shape, want_resample = SHAPES[shape]
    for f, (x, y) in enumerate(zip(ra, rb)):
        assert_same(x, y, (shape, state, f))
        print(shape, state, f, "shape", shapes[f], "refined", refined(x[4]))
        assert shapes[f][0] == shapes[f][1] == want_shape, (shape, state, f, shapes[f])
        if want_resample is not None:
            assert shapes[f][2] == want_resample, (shape, state, f, shapes[f])
    assert any(refined(x[4]) for x in ra)  # the stream tracks: Gauss-Newton had work
    assert fallbacks == 0
    assert pa == pb


@pytest.mark.parametrize("M,B", [(4, 12), (12, 40)])
def test_other_marker_buckets(M, B):
    ra, rb, shapes, fallbacks, pa, pb = run_twins("frame2", "f32", M, B)
    for f, (x, y) in enumerate(zip(ra, rb)):
        assert_same(x, y, (M, f))
    assert any(refined(x[4]) for x in ra) and fallbacks == 0 and pa == pb


@pytest.mark.parametrize("case", [(shape, state, 5, 20) for shape in SHAPES for state in STATES]
                         + [("frame2", "f32", 4, 12), ("frame2", "f32", 12, 40)])
def test_device_equals_host(case):
    shape, state, M, B = case
    st = stream(M, B)
    _, rb, *_ = run_twins(shape, state, M, B)
    for fr, res in zip(st.frames, rb):
        assert host_tail(st, fr.blobs, res) == res[1:4], (case, fr.index)


# ------------------------------------------------------------------------------------------ case 3: iteration rounds
@pytest.mark.parametrize("force_iters", [3, 20])
def test_iteration_rounds(force_iters):
    """Two-launch frames whose exit rule is held off: several finishing launches, each followed by a tail, of which
    only the last finds a finished record."""
    st = stream()
    a, b = engine(700, st, fused=0), engine(700, st, fused=0)
    try:
        for fr in st.frames[:2]:
            x = two_call(a, frame_in(a, fr, force_iters=force_iters))
            y = fused_call(b, frame_in(b, fr, force_iters=force_iters))
            assert x[4].iters == force_iters and y[4].iters == force_iters
            assert_same(x, y, (force_iters, fr.index))
        assert b.info(pf.INFO_TAIL_FALLBACKS) == 0
        assert a.get_particles(1).tobytes() == b.get_particles(1).tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------- case 4: rejected frames
@pytest.mark.parametrize("case", ["no_blobs", "far_blobs"])
@pytest.mark.parametrize("fused", [2, 0])
def test_rejected_frames(case, fused):
    st = stream()
    blobs = np.zeros((0, 2)) if case == "no_blobs" else np.array([[5000.0 + 7 * i, 6000.0 + 3 * i] for i in range(20)])
    a, b = engine(700, st, fused=fused), engine(700, st, fused=fused)
    try:
        fr = st.frames[0]
        x, y = two_call(a, frame_in(a, fr, blobs=blobs)), fused_call(b, frame_in(b, fr, blobs=blobs))
        assert y[4].flag_fail == pf.FLAG_REINIT
        assert_same(x, y, case)
        assert empty_summary(y[1]) and untouched(y)
        assert host_tail(st, blobs, y) == y[1:4]
        # the next frame is a tracked one again on both
        fr = st.frames[1]
        assert_same(two_call(a, frame_in(a, fr)), fused_call(b, frame_in(b, fr)), (case, "next"))
        assert b.info(pf.INFO_TAIL_FALLBACKS) == 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ case 5: bank blobs
def test_bank_blobs():
    st = stream()
    engs = [engine(700, st) for _ in range(3)]
    a, b, c = engs
    try:
        b.stage_blob_bank([fr.blobs for fr in st.frames])
        for fr in st.frames[:3]:
            x = two_call(a, frame_in(a, fr))
            y = fused_call(b, frame_in(b, fr, bank_frame=fr.index))
            z = fused_call(c, frame_in(c, fr))
            assert_same(x, y, ("bank", fr.index))
            assert_same(y, z, ("bank against list", fr.index))
        assert refined(x[4]) and b.info(pf.INFO_TAIL_FALLBACKS) == 0
    finally:
        for e in engs:
            e.close()


# ----------------------------------------------------------------------------------------- case 6: refine parameters
@pytest.mark.parametrize("revert", [1, 0])
def test_refine_parameters(revert):
    st = stream()
    prm = pf.default_refine_params()
    prm.max_iter, prm.revert_on_divergence = 1, revert
    a, b = engine(700, st), engine(700, st)
    try:
        for fr in st.frames[:2]:
            x, y = two_call(a, frame_in(a, fr), prm), fused_call(b, frame_in(b, fr), prm)
            assert_same(x, y, (revert, fr.index))
            assert host_tail(st, fr.blobs, y, prm) == y[1:4]
            row = pf.RefineRow.from_buffer_copy(y[2])
            assert refined(y[4]) and row.iters == 1 and row.status in (pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED)
    finally:
        a.close()
        b.close()


# -------------------------------------------------------------------------------------------- case 7: bad parameters
def test_bad_parameters_change_nothing():
    st = stream()
    a, b = engine(700, st), engine(700, st)
    try:
        assert_same(two_call(a, frame_in(a, st.frames[0])), fused_call(b, frame_in(b, st.frames[0])), 0)
        for field, value in (("max_iter", 0), ("max_iter", 10001), ("converged", -1.0), ("converged", float("nan"))):
            prm = pf.default_refine_params()
            setattr(prm, field, value)
            with pytest.raises(pf.PFError) as err:
                b.step_refine(frame_in(b, st.frames[1]), params=prm)
            assert err.value.code == pf.E_ARG and "step_refine" in str(err.value)
        for fr in st.frames[1:3]:
            assert_same(two_call(a, frame_in(a, fr)), fused_call(b, frame_in(b, fr)), fr.index)
        assert a.get_particles(1).tobytes() == b.get_particles(1).tobytes()
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------------------------------- case 9: recovery
@pytest.mark.parametrize("fused", [2, 0])
def test_recovery_path(fused):
    st = stream()
    a, b = engine(700, st, fused=fused), engine(700, st, fused=fused)
    try:
        b.set_option(pf.OPT_DIAG, pf.DIAG_TAIL_MISS)
        x, y = two_call(a, frame_in(a, st.frames[0])), fused_call(b, frame_in(b, st.frames[0]))
        assert refined(y[4])
        assert_same(x, y, "missed")
        assert b.info(pf.INFO_TAIL_FALLBACKS) == 1
        b.set_option(pf.OPT_DIAG, 0)
        assert_same(two_call(a, frame_in(a, st.frames[1])), fused_call(b, frame_in(b, st.frames[1])), "clean")
        assert b.info(pf.INFO_TAIL_FALLBACKS) == 1
        assert a.get_particles(1).tobytes() == b.get_particles(1).tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------- the batch
def summary_bytes(d):
    return b"".join([np.array([d[k] for k in INT_KEYS], dtype=np.int64).tobytes(), d["best_row"].tobytes(),
                     d["best_cov"].tobytes()])


def batch_two_call(engs, frames, blob_lists, params=None):
    """step_multi, then refine_multi with K = 1 for the streams that are refined and K = 0 for the others."""
    outs = pf.Engine.step_multi(engs, frames)
    poses = [np.array(o.winner_pose).reshape(1, 12) if refined(o) else np.zeros((0, 12)) for o in outs]
    pairs = [np.array(o.corr, dtype=np.uint32).reshape(1, pf.MAX_MARKERS, 2) if refined(o)
             else np.zeros((0, pf.MAX_MARKERS, 2), dtype=np.uint32) for o in outs]
    res = pf.Engine.refine_multi(engs, poses, pairs, blob_lists, params=params, want_rows=True, want_cov=True)
    return outs, res


def batch_fused(engs, frames, params=None):
    S = len(engs)
    rows = (pf.RefineRow * S).from_buffer_copy(bytes([ROW_FILL]) * (S * C.sizeof(pf.RefineRow)))
    cov = np.full((S, 36), COV_FILL)
    return pf.Engine.step_refine_multi(engs, frames, params=params, rows=rows, cov=cov)


def assert_batch_same(two, fusedr, tag):
    (outs_a, res_a), (outs_b, gns, rows, cov) = two, fusedr
    for s in range(len(outs_a)):
        assert bytes(outs_a[s]) == bytes(outs_b[s]), (tag, s, "frame_out")
        assert summary_bytes(res_a[s]) == summary_bytes(gns[s].as_dict()), (tag, s, "summary")
        if refined(outs_a[s]):
            assert bytes(rows[s]) == res_a[s]["rows"].tobytes(), (tag, s, "row")
            assert cov[s].tobytes() == res_a[s]["cov"].tobytes(), (tag, s, "cov")
        else:
            assert gns[s].n == 0 and gns[s].best == -1, (tag, s)
            assert bytes(rows[s]) == bytes([ROW_FILL]) * C.sizeof(pf.RefineRow) and (cov[s] == COV_FILL).all(), (tag, s)


def test_batch_mixed_streams():
    """S = 3, F32, N = (300, 700, 2048): stream 1 has no blobs (rejected), stream 2 runs three iterations, so the batch
    takes further rounds for it while the others' records are already finished."""
    Ns = (300, 700, 2048)
    sts = [stream(seed=s) for s in range(3)]
    ea = [engine(N, st, seed=s) for s, (N, st) in enumerate(zip(Ns, sts))]
    eb = [engine(N, st, seed=s) for s, (N, st) in enumerate(zip(Ns, sts))]
    try:
        for f in range(2):
            def frames(engs):
                return [frame_in(engs[0], sts[0].frames[f]),
                        frame_in(engs[1], sts[1].frames[f], blobs=np.zeros((0, 2))),
                        frame_in(engs[2], sts[2].frames[f], force_iters=3)]
            blob_lists = [sts[0].frames[f].blobs, np.zeros((0, 2)), sts[2].frames[f].blobs]
            two, fusedr = batch_two_call(ea, frames(ea), blob_lists), batch_fused(eb, frames(eb))
            assert_batch_same(two, fusedr, f)
            assert refined(two[0][0]) and not refined(two[0][1]) and two[0][2].iters == 3
        assert all(e.info(pf.INFO_TAIL_FALLBACKS) == 0 for e in eb)
        for x, y in zip(ea, eb):
            assert x.get_particles(1).tobytes() == y.get_particles(1).tobytes()
    finally:
        for e in ea + eb:
            e.close()


def test_batch_64_streams_member_ordering_and_errors():
    """S = 64 x N = 256 against the two-call batch; then a batch with a bad params[2] (refused whole, nothing
    launched: the next batch still equals the twins'); then a member's own step_refine after a batch."""
    S, N = 64, 256
    sts = [stream(seed=s) for s in range(S)]
    ea = [engine(N, st, seed=s) for s, st in enumerate(sts)]
    eb = [engine(N, st, seed=s) for s, st in enumerate(sts)]
    try:
        def frames(engs, f):
            return [frame_in(e, st.frames[f]) for e, st in zip(engs, sts)]
        blob_lists = lambda f: [st.frames[f].blobs for st in sts]  # noqa: E731
        two, fusedr = batch_two_call(ea, frames(ea, 0), blob_lists(0)), batch_fused(eb, frames(eb, 0))
        assert_batch_same(two, fusedr, "64")
        assert sum(refined(o) for o in two[0]) >= S // 2
        # error paths: params[2] is bad
        prms = [pf.default_refine_params() for _ in range(S)]
        prms[2].max_iter = 0
        with pytest.raises(pf.PFError) as err:
            pf.Engine.step_refine_multi(eb, frames(eb, 1), params=prms)
        assert err.value.code == pf.E_ARG and str(err.value).find("step_refine_multi: stream 2: ") >= 0
        with pytest.raises(pf.PFError) as err:  # pfmpe_step_multi's own checks under the new name
            pf.Engine.step_refine_multi([eb[0], eb[1], eb[0]], frames(eb, 1)[:3])
        assert "step_refine_multi: stream 2: " in str(err.value)
        two, fusedr = batch_two_call(ea, frames(ea, 1), blob_lists(1)), batch_fused(eb, frames(eb, 1))
        assert_batch_same(two, fusedr, "after the refused batches")
        # a member on its own stream after the batches
        s = 5
        x = two_call(ea[s], frame_in(ea[s], sts[s].frames[2]))
        y = fused_call(eb[s], frame_in(eb[s], sts[s].frames[2]))
        assert_same(x, y, "member")
        assert all(e.info(pf.INFO_TAIL_FALLBACKS) == 0 for e in eb)
        assert ea[s].get_particles(1).tobytes() == eb[s].get_particles(1).tobytes()
        assert ea[0].get_particles(1).tobytes() == eb[0].get_particles(1).tobytes()
    finally:
        for e in ea + eb:
            e.close()


def test_batch_recovery_path():
    sts = [stream(seed=s) for s in range(3)]
    ea = [engine(300, st, seed=s) for s, st in enumerate(sts)]
    eb = [engine(300, st, seed=s) for s, st in enumerate(sts)]
    try:
        eb[0].set_option(pf.OPT_DIAG, pf.DIAG_TAIL_MISS)  # the leader's switch
        fa = [frame_in(e, st.frames[0]) for e, st in zip(ea, sts)]
        fb = [frame_in(e, st.frames[0]) for e, st in zip(eb, sts)]
        assert_batch_same(batch_two_call(ea, fa, [st.frames[0].blobs for st in sts]), batch_fused(eb, fb), "missed")
        assert [e.info(pf.INFO_TAIL_FALLBACKS) for e in eb] == [1, 1, 1]
    finally:
        for e in ea + eb:
            e.close()


# ----------------------------------------------------------------------------------------------------- the bracket
def test_tail_is_one_aux_bracket_on_one_launch_frames():
    st = stream()
    b = engine(700, st)
    try:
        b.set_option(pf.OPT_TIMING, 1)
        for fr in st.frames[:3]:
            b.step_refine(frame_in(b, fr))
        assert b.info(pf.INFO_LAST_SHAPE) == pf.SHAPE_FRAME2
        stats = b.kernel_stats()
        assert stats["aux"][0] == 3 and stats["k_frame"][0] == 3 and stats["aux"][1] > 0.0
    finally:
        b.close()
