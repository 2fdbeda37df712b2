"""pfmpe_cloud_stats_multi: the cloud statistics of S entries in one batch.

A batch entry returns the bytes of its own single call: every comparison with pfmpe_cloud_stats here is of the raw
480-byte records.  Covered: every state type, particle counts on both sides of every wave and block boundary, a cloud
larger than the 1,024-block grid (the entry's own grid stride) next to small ones, priors in particle order and read
through owner indices, a context in several entries, reversed order, S = 1 and S = 64, members whose latest work is on
another stream, a degenerate entry beside normal ones, repeatability and freedom from side effects, and every
argument error.  The single call is the batch of one (it shares the leader's batch scratch, which has a test), so the
batch is also held against the numpy restatement (tests/cloud_ref.py) at that file's tolerance: one entry per state,
and every entry of one mixed batch."""
import ctypes as C
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from pf_monocular_pose_estimator_amd import _capi
from test_gpu_parity import make_engine

import cloud_ref

pytestmark = pytest.mark.gpu

STATES = {"f64": pf.STATE_F64, "f32": pf.STATE_F32, "f16": pf.STATE_F16}
W, P = pf.CLOUD_WEIGHTED, pf.CLOUD_POSTERIOR
DP = C.POINTER(C.c_double)


@functools.lru_cache(maxsize=None)
def _stream():
    return syn.make_stream(syn.StreamConfig("t", M=5, B=50, N=1000), 3)


class Obj:
    """One tracked object: an engine with a prior of its own, and the frames that drive it."""

    def __init__(self, i, N, state, fused=2, with_prior=True):
        self.i, self.N = i, N
        self.st = _stream()
        self.eng = make_engine(N, self.st.markers, self.st.K, state, pf.RNG_PHILOX, fused=fused)
        self.prior0 = None
        self.out = None
        if with_prior:
            prior = syn.initial_prior_fast(syn.to44(self.st.frames[0].current_pose), N, seed=7 + i)
            self.prior0 = prior[0].reshape(12).copy()
            self.eng.set_prior(prior)

    def frame(self, f, blobs=None):
        fr = self.st.frames[f]
        blobs = fr.blobs if blobs is None else blobs
        return self.eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=blobs, dt=fr.dt,
                                   seed=900 + 13 * self.i + f, frame_idx=f)

    def step(self, f, blobs=None):
        self.out = self.eng.step(self.frame(f, blobs))
        return self.out

    def ref(self):
        """cloud_stats' default reference: the last step's winner when it resampled, else its most likely pose; the
        first particle of the prior before any step"""
        if self.out is None:
            return self.prior0
        return np.array(self.out.winner_pose if self.out.resampled else self.out.most_likely_pose)

    def single(self, which, ref=None):
        out = _capi.CloudOut()
        r = np.ascontiguousarray(self.ref() if ref is None else ref, dtype=np.float64)
        rc = self.eng.lib.pfmpe_cloud_stats(self.eng.ctx, which, r.ctypes.data_as(DP), C.byref(out))
        assert rc == pf.OK, self.eng.last_error()
        return bytes(out)


def raw_batch(entries):
    """entries: (Obj, which) or (Obj, which, ref) -> the raw records of one pfmpe_cloud_stats_multi call"""
    S = len(entries)
    ctxs = (C.c_void_p * S)(*[e[0].eng.ctx.value for e in entries])
    arr_in = (_capi.CloudIn * S)(*[pf.Engine.make_cloud_in(e[1], e[0].ref() if len(e) < 3 else e[2]) for e in entries])
    arr_out = (_capi.CloudOut * S)()
    lead = entries[0][0].eng
    rc = lead.lib.pfmpe_cloud_stats_multi(ctxs, S, arr_in, arr_out)
    assert rc == pf.OK, lead.last_error()
    return [bytes(o) for o in arr_out]


def equals_singles(entries, what, twins=None):
    got = raw_batch(entries)
    for s, (e, g) in enumerate(zip(entries, got)):
        o = e[0] if twins is None else twins[e[0].i]
        assert g == o.single(e[1], None if len(e) < 3 else e[2]), (what, "entry", s, "N", e[0].N, "which", e[1])
    return got


def as_dict(raw):
    return _capi.CloudOut.from_buffer_copy(raw).as_dict()


def close(objs):
    for o in objs:
        o.eng.close()


@pytest.mark.parametrize("state", ["f64", "f32", "f16"])
def test_batch_equals_single(state):
    """a lone lane, a partial wave, a full wave, a block plus one, a tail that is no multiple of 64, and 17 blocks: the
    priors alone, then both sets of every context in one batch after two steps of each (every context twice)"""
    objs = [Obj(i, N, STATES[state]) for i, N in enumerate((1, 63, 64, 257, 1000, 4097))]
    try:
        got = equals_singles([(o, P) for o in objs], (state, "prior"))
        o = objs[4]
        cloud_ref.check(as_dict(got[4]), cloud_ref.stats(o.eng.get_particles(1), None, o.ref()))
        assert [as_dict(g)["n"] for g in got] == [o.N for o in objs]
        for o in objs:
            o.step(0)
            o.step(1)
        entries = [(o, which) for o in objs for which in (W, P)]
        got = equals_singles(entries, (state, "after two steps"))
        assert len(got) == 12 and len(set(got)) == 12
        o = objs[5]
        assert o.out.resampled
        cloud_ref.check(as_dict(got[10]), cloud_ref.stats(o.eng.get_particles(0), o.eng.get_weights(), o.ref()))
        cloud_ref.check(as_dict(got[11]), cloud_ref.stats(o.eng.get_particles(1), None, o.ref()))
    finally:
        close(objs)


@pytest.mark.parametrize("state", ["f32", "f16"])
def test_grid_stride_and_owner_gather(state):
    """300,001 particles are 1,172 particle blocks on the entry's 1,024-block grid: its lanes stride by its own grid,
    not by the batch's; two priors read through owner indices next to one in particle order"""
    objs = [Obj(0, 300_001, STATES[state], fused=0), Obj(1, 5000, STATES[state], fused=0),
            Obj(2, 3000, STATES[state], fused=0)]
    try:
        objs[2].eng.set_option(pf.OPT_DEFER_RESAMPLE, 0)
        for o in objs:
            assert o.step(0).resampled
        assert objs[0].eng.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS
        assert objs[1].eng.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS
        assert objs[2].eng.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_BLOCKS
        plan, total = pf.host_cloud_plan([o.N for o in objs for _ in (W, P)])
        assert plan[0]["blocks"] == 1024 and total == 2 * (1024 + 20 + 12)
        equals_singles([(o, which) for o in objs for which in (W, P)], state)
        equals_singles([(o, which) for which in (P, W) for o in objs[::-1]], (state, "large entry last"))
    finally:
        close(objs)


def test_mixed_batch_against_numpy():
    """One mixed batch held against the numpy restatement on each member's own read-backs, not against the single
    call: both sets of one context, a second context of another N, and a context twice with two reference poses
    (the default one and a particle of its own set, so both lie inside the cloud).  cloud_ref.check's 1e-9 rule
    holds with room: the sums' rounding is at most N * 2^-53 = 5e-13 at N = 4,097."""
    objs = [Obj(i, N, pf.STATE_F32) for i, N in enumerate((1000, 4097, 257))]
    A, B, Cc = objs
    try:
        for o in objs:
            o.step(0)
        sets = {o.i: {W: (o.eng.get_particles(0), o.eng.get_weights()), P: (o.eng.get_particles(1), None)}
                for o in objs}
        own = sets[Cc.i][P][0][-1].reshape(12).copy()
        entries = [(A, W, A.ref()), (A, P, A.ref()), (B, W, B.ref()), (Cc, P, Cc.ref()), (Cc, P, own)]
        got = raw_batch(entries)
        assert len(set(got)) == len(got)
        for (o, which, ref), g in zip(entries, got):
            poses, w = sets[o.i][which]
            cloud_ref.check(as_dict(g), cloud_ref.stats(poses, w, ref))
    finally:
        close(objs)


@pytest.mark.parametrize("state", ["f32", "f16"])
def test_single_and_batch_share_scratch(state):
    """The single call is a batch of one in the leader's batch scratch: a batch of three entries (the large context,
    the small one, the large one again), the small context's single calls, the large one's, then the batch again.
    Every record is the one a fresh pair of engines in the same state returns as its first statistics call."""
    made = []

    def fresh():
        pair = [Obj(0, 257, STATES[state]), Obj(1, 4097, STATES[state])]
        made.extend(pair)
        for o in pair:
            o.step(0)
        return pair

    def entries(small, large):
        return [(large, W), (small, P), (large, P)]

    try:
        want_batch = raw_batch(entries(*fresh()))
        want = {(i, which): fresh()[i].single(which) for i in (0, 1) for which in (W, P)}
        small, large = fresh()
        assert raw_batch(entries(small, large)) == want_batch
        for o in (small, large):
            for which in (W, P):
                assert o.single(which) == want[o.i, which], (o.N, which)
        assert raw_batch(entries(small, large)) == want_batch
    finally:
        close(made)


def test_order_and_membership():
    objs = [Obj(i, N, pf.STATE_F32) for i, N in enumerate((700, 64, 1025))]
    many = []
    try:
        fwd = equals_singles([(o, P) for o in objs], "forward")
        rev = raw_batch([(o, P) for o in objs[::-1]])
        assert fwd == rev[::-1]
        for o, g in zip(objs, fwd):
            assert raw_batch([(o, P)]) == [g], "S = 1"
        many = [Obj(i, 3 + 5 * i, pf.STATE_F32) for i in range(pf.CLOUD_MAX_STREAMS)]  # N = 3 .. 318
        got = equals_singles([(o, P) for o in many], "S = 64")
        assert len(got) == pf.CLOUD_MAX_STREAMS and [as_dict(g)["n"] for g in got] == [o.N for o in many]
        # the binding: the dicts the single call returns
        a = pf.Engine.cloud_stats_multi([o.eng for o in objs], [P] * 3, [o.ref() for o in objs])
        for o, d in zip(objs, a):
            b = o.eng.cloud_stats(P, ref=o.ref())
            assert d.keys() == b.keys()
            for k in d:
                assert np.array_equal(np.asarray(d[k]), np.asarray(b[k])), k
    finally:
        close(objs + many)


def test_members_with_work_on_other_streams():
    """a statistics batch led by C right after a step batch led by A, and one led by A right after a solo step of B:
    everything equals a twin set of engines driven by single calls only"""
    sizes = (20_000, 33_333, 9000)
    objs = [Obj(i, N, pf.STATE_F32, fused=0) for i, N in enumerate(sizes)]
    twin = [Obj(i, N, pf.STATE_F32, fused=0) for i, N in enumerate(sizes)]
    A, B, Cc = objs
    try:
        outs = pf.Engine.step_multi([o.eng for o in objs], [o.frame(0) for o in objs])
        for o, out in zip(objs, outs):
            o.out = out
        for t in twin:
            t.step(0)
        equals_singles([(Cc, W), (A, W), (B, P), (Cc, P), (A, P), (B, W)], "after step_multi", twins=twin)
        assert np.array_equal(B.eng.get_particles(1), twin[1].eng.get_particles(1))
        B.step(1)
        got = raw_batch([(A, W), (B, W), (Cc, W), (A, P), (B, P), (Cc, P)])
        twin[1].step(1)
        for g, (t, which) in zip(got, [(t, which) for which in (W, P) for t in twin]):
            assert g == t.single(which), ("after solo step", t.i, which)
        assert np.array_equal(B.eng.get_particles(0), twin[1].eng.get_particles(0))
        assert np.array_equal(B.eng.get_particles(1), twin[1].eng.get_particles(1))
    finally:
        close(objs + twin)


def test_degenerate_entry_beside_normal_ones():
    """a frame without blobs takes the re-initialisation branch with every weight zero"""
    objs = [Obj(i, N, pf.STATE_F32) for i, N in enumerate((1000, 1000, 777))]
    try:
        objs[0].step(0)
        out = objs[1].step(0, blobs=np.zeros((0, 2)))
        assert out.prob_sum == 0 and not out.resampled
        objs[2].step(0)
        got = equals_singles([(objs[0], W), (objs[1], W), (objs[2], W), (objs[1], P), (objs[0], P)], "degenerate")
        d = as_dict(got[1])
        assert d["degenerate"] == 1 and d["n"] == 1000 and d["wsum"] == 0 and d["ess"] == 0
        assert np.array_equal(d["mean_pose"], np.array(out.most_likely_pose))
        assert np.array_equal(d["mean_twist"], np.zeros(6)) and np.array_equal(d["cov"], np.zeros((6, 6)))
        for s in (0, 2, 3, 4):
            assert as_dict(got[s])["degenerate"] == 0 and as_dict(got[s])["wsum"] > 0
    finally:
        close(objs)


def test_repeatable_and_side_effect_free():
    """two batches return the same bytes; a 3-frame step_multi run with a statistics batch after every frame equals
    the run without it in every frame record, particle set and weight vector"""
    sizes = (20_000, 9000, 4097)
    runs = []
    for with_stats in (True, False):
        objs = [Obj(i, N, pf.STATE_F32, fused=0) for i, N in enumerate(sizes)]
        snaps = []
        try:
            for f in range(3):
                outs = pf.Engine.step_multi([o.eng for o in objs], [o.frame(f) for o in objs])
                for o, out in zip(objs, outs):
                    o.out = out
                if with_stats:
                    entries = [(o, which) for o in objs for which in (W, P)]
                    assert raw_batch(entries) == raw_batch(entries)
                snaps.append([{"out": out.as_dict(), "w": o.eng.get_weights(), "p0": o.eng.get_particles(0),
                               "p1": o.eng.get_particles(1)} for o, out in zip(objs, outs)])
        finally:
            close(objs)
        runs.append(snaps)
    for f, (xs, ys) in enumerate(zip(*runs)):
        for i, (x, y) in enumerate(zip(xs, ys)):
            for k, v in x["out"].items():
                assert np.array_equal(np.asarray(v), np.asarray(y["out"][k])), (f, i, k)
            for k in ("w", "p0", "p1"):
                assert np.array_equal(x[k], y[k]), (f, i, k)


def test_errors_leave_out_untouched():
    lib = pf.load()
    objs = [Obj(i, 300 + i, pf.STATE_F32) for i in range(3)]
    other = Obj(3, 300, pf.STATE_F64)
    bare = Obj(4, 300, pf.STATE_F32, with_prior=False)
    A, B, Cc = objs
    ref = A.prior0
    SENTINEL = b"\xa5" * C.sizeof(_capi.CloudOut)

    def call(members, whichs=None, refs=None, S=None, null_in=False, null_out=False, null_ctxs=False):
        S = len(members) if S is None else S
        n = max(len(members), 1)
        whichs = [P] * n if whichs is None else whichs
        refs = [ref] * n if refs is None else refs
        ctxs = (C.c_void_p * n)(*[m.eng.ctx.value if m is not None else None for m in members])
        arr_in = (_capi.CloudIn * n)(*[pf.Engine.make_cloud_in(w, r) for w, r in zip(whichs, refs)])
        arr_out = (_capi.CloudOut * n)()
        C.memset(arr_out, 0xA5, C.sizeof(arr_out))
        rc = lib.pfmpe_cloud_stats_multi(None if null_ctxs else ctxs, S, None if null_in else arr_in,
                                         None if null_out else arr_out)
        return rc, all(bytes(o) == SENTINEL for o in arr_out), A.eng.last_error()

    try:
        A.step(0)
        nan_ref = ref.copy()
        nan_ref[7] = np.nan
        inf_ref = ref.copy()
        inf_ref[0] = np.inf
        pre = "cloud_stats_multi: "
        cases = [
            ("state type", call([A, other, B]), pf.E_ARG, pre + "stream 1: "),
            ("no particle set", call([A, bare]), pf.E_STATE, pre + "stream 1: "),
            ("weighted before the first step", call([A, A, B], whichs=[W, P, W]), pf.E_STATE, pre + "stream 2: "),
            ("bad which", call([A, B, Cc], whichs=[P, P, 2]), pf.E_ARG, pre + "stream 2: "),
            ("negative which", call([A, B], whichs=[P, -1]), pf.E_ARG, pre + "stream 1: "),
            ("nan ref", call([A, B], refs=[ref, nan_ref]), pf.E_ARG, pre + "stream 1: "),
            ("inf ref", call([A, B], refs=[inf_ref, ref]), pf.E_ARG, pre + "stream 0: "),
            ("null member", call([A, None]), pf.E_ARG, pre + "stream 1: "),
            ("S = 65", call([A] * 65), pf.E_CAP, pre),
            ("null in", call([A, B], null_in=True), pf.E_ARG, pre),
            ("null out", call([A, B], null_out=True), pf.E_ARG, pre),
        ]
        for name, (rc, untouched, text), code, prefix in cases:
            assert rc == code, (name, rc)
            assert untouched, name
            assert text.startswith(prefix), (name, text)
        # without a leader there is nobody to hold a text
        before = A.eng.last_error()
        for name, (rc, untouched, text) in [("S = 0", call([A, B], S=0)), ("S < 0", call([A, B], S=-3)),
                                            ("null ctxs", call([A, B], null_ctxs=True)),
                                            ("null leader", call([None, B]))]:
            assert rc == pf.E_ARG and untouched, name
            assert text == before, name
        with pytest.raises(pf.PFError) as ei:
            pf.Engine.cloud_stats_multi([A.eng, bare.eng], [P, P], [ref, ref])
        assert ei.value.code == pf.E_STATE
        with pytest.raises(ValueError):
            pf.Engine.cloud_stats_multi([A.eng, B.eng], [P], [ref, ref])
        with pytest.raises(ValueError):
            pf.Engine.cloud_stats_multi([A.eng, B.eng], [P, P], [ref])
        # a valid batch afterwards (A twice: both of its sets)
        equals_singles([(A, W), (B, P, ref), (Cc, P, ref), (A, P)], "after the errors")
    finally:
        close(objs + [other, bare])
