"""pfmpe_refine_multi on the device: the Gauss-Newton refinement of S streams' hypotheses as one batch.

The reference of every case is the S single refine_poses calls on the same engines: existing code, pinned to
pfmpe_host_optimise_pose and the oracle by test_gpu_refine.py.  Equality is of bytes (tobytes() of rows, cov, best_row,
best_cov, and the integer fields): a lane of the batch runs the same function on the same numbers, every summed
quantity of a summary is an integer and the best key is a total order, so no tolerance is involved.  Every bad input
is refused on the host before a launch.
"""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

import refine_ref as rr

pytestmark = pytest.mark.gpu

STATE_OF = {"A": pf.STATE_F64, "B": pf.STATE_F32, "C": pf.STATE_F16}
INT_KEYS = ("n", "n_with_pairs", "n_converged", "n_cap_kept", "n_cap_reverted", "iters_total", "iters_max", "best")
U32 = C.POINTER(C.c_uint32)
DP = C.POINTER(C.c_double)


def make_engine(name, max_particles=512, state=None, max_blobs=pf.MAX_BLOBS, model=True):
    markers, K = rr.cloud(name)[:2]
    eng = pf.Engine(device=0, max_particles=max_particles, max_blobs=max_blobs,
                    state_dtype=STATE_OF[name] if state is None else state)
    if model:
        eng.set_model(markers, K)
    eng.set_params(pf.default_params())
    return eng


def hyps(name, k, start=0):
    """k hypotheses of a cloud with at least one pair each, from the start-th such row on: (poses, pairs, blobs),
    copies (the shared clouds stay as they are)."""
    _, _, blobs, poses, pairs, oref = rr.cloud(name)
    sel = np.flatnonzero(oref["n_pairs"] > 0)[start:start + k]
    assert len(sel) == k
    return poses[sel].copy(), pairs[sel].copy(), blobs.copy()


def summary_bytes(res):
    return b"".join([np.array([res[k] for k in INT_KEYS], dtype=np.int64).tobytes(), res["best_row"].tobytes(),
                     res["best_cov"].tobytes()])


def singles(engs, poses, pairs, blobs=None, bank=None, params=None):
    """The reference: one refine_poses call per stream."""
    S = len(engs)
    res = []
    for s in range(S):
        p = params[s] if isinstance(params, (list, tuple)) else params
        res.append(engs[s].refine_poses(poses[s], pairs[s], blobs=None if blobs is None else blobs[s],
                                        bank_frame=-1 if bank is None else bank[s], params=p, want_cov=True))
    return res


def same(got, ref, tag=""):
    """Every stream of a batch against its single call, byte for byte."""
    assert len(got) == len(ref)
    for s, (g, r) in enumerate(zip(got, ref)):
        for k in INT_KEYS:
            assert g[k] == r[k], (tag, s, k, g[k], r[k])
        assert summary_bytes(g) == summary_bytes(r), (tag, s)
        if "rows" in g:
            assert g["rows"].tobytes() == r["rows"].tobytes(), (tag, s)
        if "cov" in g:
            assert g["cov"].tobytes() == r["cov"].tobytes(), (tag, s)


def close_all(engs):
    for e in set(engs):
        e.close()


# ----------------------------------------------------------------------------------------------------- identity
def test_identity_mixed_everything():
    """A (F64, 5 LEDs / 20 blobs), B (F32, 4 / 12), C (F16, 12 / 40) with K = (1, 65, 300): waves hold lanes of two
    streams, stream C crosses a block boundary."""
    names, ks = ("A", "B", "C"), (1, 65, 300)
    engs = [make_engine(n) for n in names]
    try:
        poses, pairs, blobs = zip(*[hyps(n, k) for n, k in zip(names, ks)])
        ref = singles(engs, poses, pairs, blobs)
        full = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_rows=True, want_cov=True)
        same(full, ref, "rows+cov")
        assert [r["n"] for r in full] == list(ks)
        assert all("rows" in r and "cov" in r and len(r["rows"]) == k for r, k in zip(full, ks))
        rows_only = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_rows=True, want_cov=False)
        same(rows_only, ref, "rows")
        assert all("cov" not in r for r in rows_only)
        neither = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_rows=False, want_cov=False)
        same(neither, ref, "summaries")
        assert all("rows" not in r and "cov" not in r for r in neither)
        for a, b, c in zip(full, rows_only, neither):
            assert summary_bytes(a) == summary_bytes(b) == summary_bytes(c)
        # the cloud has work for the summary: a best hypothesis in every stream
        assert all(r["best"] >= 0 and r["n_with_pairs"] == k for r, k in zip(full, ks))
    finally:
        close_all(engs)


# ------------------------------------------------------------------------------------------- the real frame shape
def test_frame_shape_64_streams():
    """S = 64 engines (max_particles 16, configurations cycling A / B / C), one hypothesis each; then K = 0 on every
    other stream: the single call's empty summary, and rows that are not touched."""
    S = 64
    names = [("A", "B", "C")[s % 3] for s in range(S)]
    engs = [make_engine(n, max_particles=16) for n in names]
    try:
        poses, pairs, blobs = map(list, zip(*[hyps(n, 1, start=s) for s, n in enumerate(names)]))
        ref = singles(engs, poses, pairs, blobs)
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
        same(got, ref, "K=1")
        assert all(r["n"] == 1 and r["best"] == 0 for r in got)
        # every other stream without a hypothesis
        for s in range(1, S, 2):
            poses[s], pairs[s] = poses[s][:0], pairs[s][:0]
        ref = singles(engs, poses, pairs, blobs)
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
        same(got, ref, "K=0/1")
        for s in range(1, S, 2):
            assert got[s]["n"] == 0 and got[s]["best"] == -1 and len(got[s]["rows"]) == 0
            assert not np.frombuffer(got[s]["best_row"].tobytes(), dtype=np.uint8).any() and not got[s]["best_cov"].any()
        # rows / cov arrays of a K = 0 stream are not written: hand the call prefilled ones
        lib = pf.load()
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engs])
        ins, outs = (pf.RefineIn * S)(), (pf.RefineOut * S)()
        keep = []
        rows = [np.full(1, 0x5A, dtype=np.uint8).repeat(128) for _ in range(S)]
        covs = [np.full(36, -7.25) for _ in range(S)]
        for s in range(S):
            ai, kb = pf.Engine._assoc_in(blobs[s], -1)
            po, pr = np.ascontiguousarray(poses[s]), np.ascontiguousarray(pairs[s])
            keep.append((kb, po, pr))
            ins[s].blobs, ins[s].K = ai, len(po)
            if len(po):
                ins[s].poses, ins[s].corr = po.ctypes.data_as(DP), pr.ctypes.data_as(U32)
        rp = (C.c_void_p * S)(*[r.ctypes.data for r in rows])
        cp = (DP * S)(*[c.ctypes.data_as(DP) for c in covs])
        assert lib.pfmpe_refine_multi(ctxs, S, ins, None, outs, rp, cp) == pf.OK
        for s in range(S):
            if s % 2:
                assert (rows[s] == 0x5A).all() and (covs[s] == -7.25).all(), s
            else:
                assert rows[s].tobytes() == ref[s]["rows"].tobytes() and covs[s].tobytes() == ref[s]["cov"].tobytes(), s
    finally:
        close_all(engs)


def test_all_streams_empty():
    engs = [make_engine(n, max_particles=16) for n in ("A", "B", "C")]
    try:
        blobs = [rr.cloud(n)[2] for n in ("A", "B", "C")]
        poses = [np.zeros((0, 12))] * 3
        pairs = [np.zeros((0, pf.MAX_MARKERS, 2), dtype=np.uint32)] * 3
        ref = singles(engs, poses, pairs, blobs)
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
        same(got, ref)
        for r in got:
            assert r["n"] == 0 and r["best"] == -1 and r["iters_max"] == 0 and not r["best_cov"].any()
        # without blob lists either
        got = pf.Engine.refine_multi(engs, poses, pairs)
        same(got, ref)
    finally:
        close_all(engs)


# ------------------------------------------------------------------------------------------ per-stream parameters
def test_per_stream_parameters():
    """Stream 0 default, stream 1 max_iter = 2, stream 2 max_iter = 2 without the divergence rule, on the 70-row
    selection of test_gpu_refine.py::test_list_empty_and_params; and params = NULL against explicit defaults."""
    engs = [make_engine("A", max_particles=100, state=st) for st in (pf.STATE_F64, pf.STATE_F32, pf.STATE_F16)]
    try:
        po, pr, bl = hyps("A", 70)
        poses, pairs, blobs = [po] * 3, [pr] * 3, [bl] * 3
        p1, p2 = pf.default_refine_params(), pf.default_refine_params()
        p1.max_iter = 2
        p2.max_iter = 2
        p2.revert_on_divergence = 0
        params = [pf.default_refine_params(), p1, p2]
        ref = singles(engs, poses, pairs, blobs, params=params)
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, params=params, want_cov=True)
        same(got, ref, "per stream")
        # the parameters did something, each in its stream only
        assert got[0]["n_converged"] >= 60
        assert got[1]["n_cap_kept"] + got[1]["n_cap_reverted"] >= 60 and got[1]["iters_max"] == 2
        assert got[2]["n_cap_reverted"] == 0 and got[2]["n_cap_kept"] == got[1]["n_cap_kept"] + got[1]["n_cap_reverted"]
        # NULL parameters are the defaults
        dflt = pf.Engine.refine_multi(engs, poses, pairs, blobs, params=[pf.default_refine_params()] * 3, want_cov=True)
        null = pf.Engine.refine_multi(engs, poses, pairs, blobs, params=None, want_cov=True)
        same(null, dflt, "NULL params")
        same(null, singles(engs, poses, pairs, blobs), "NULL params, singles")
    finally:
        close_all(engs)


# ------------------------------------------------------------------------------------------------- blob sources
def test_blob_sources():
    """One stream from a staged bank frame of its own context, one from a host list."""
    engs = [make_engine("A"), make_engine("B")]
    try:
        pa, ra, ba = hyps("A", 9)
        pb, rb, bb = hyps("B", 5)
        engs[0].stage_blob_bank([bb, ba])  # frame 1 holds A's blobs; frame 0 another list
        ref = singles(engs, [pa, pb], [ra, rb], blobs=[None, bb], bank=[1, -1])
        got = pf.Engine.refine_multi(engs, [pa, pb], [ra, rb], blobs_list=[None, bb], bank_frames=[1, -1], want_cov=True)
        same(got, ref, "bank + host")
        # the bank frame is the host list
        host = pf.Engine.refine_multi(engs, [pa, pb], [ra, rb], blobs_list=[ba, bb], want_cov=True)
        same(host, ref, "host + host")
    finally:
        close_all(engs)


def test_a_context_twice():
    """Two different blob lists and hypothesis sets of one context, and a second context between them."""
    a, b = make_engine("A", state=pf.STATE_F32), make_engine("B")
    try:
        p0, r0, bl = hyps("A", 7)
        p1, r1, _ = hyps("A", 66, start=100)
        moved = bl + np.array([0.75, -0.5])  # the camera's second list: another frame of the same LEDs
        pb, rb, bb = hyps("B", 3)
        engs = [a, b, a]
        ref = singles(engs, [p0, pb, p1], [r0, rb, r1], [bl, bb, moved])
        got = pf.Engine.refine_multi(engs, [p0, pb, p1], [r0, rb, r1], [bl, bb, moved], want_cov=True)
        same(got, ref)
        assert got[0]["n"] == 7 and got[2]["n"] == 66
    finally:
        close_all([a, b])


# --------------------------------------------------------------------------------------------- leader's scratch
def test_leader_scratch_grows_and_is_reused():
    """A batch of 3 hypotheses, then 366, then 3 again on the same engines: each equals its single calls, and a
    repeated call returns the same bytes."""
    names = ("A", "B", "C")
    engs = [make_engine(n) for n in names]
    try:
        for ks in ((1, 1, 1), (1, 65, 300), (1, 1, 1)):
            poses, pairs, blobs = zip(*[hyps(n, k, start=3) for n, k in zip(names, ks)])
            ref = singles(engs, poses, pairs, blobs)
            got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
            again = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
            same(got, ref, ks)
            same(again, got, ks)
    finally:
        close_all(engs)


# ---------------------------------------------------------------------------------------- nothing else changes
def stepped_engine(name, N, state, seed):
    """An engine with a prior after one step of the synthetic stream at rr.scene(name)."""
    M, B, heavy = rr.CONFIGS[name]
    cfg = syn.StreamConfig(name, M=M, B=B, N=N, heavy=heavy)
    st = syn.make_stream(cfg, 2, t0=rr.SCENE_T - cfg.dt)
    eng = pf.Engine(device=0, max_particles=N, state_dtype=state)
    eng.set_model(st.markers, st.K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_PHILOX
    eng.set_params(prm)
    eng.set_prior(st.prior(N).astype(np.float32).astype(np.float64))
    fr = st.frames[0]
    eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=seed,
                            frame_idx=0))
    return eng, st


def test_frame_state_untouched():
    """Two engines with the same prior and seed step; one goes through refine_multi as leader and as member; both step
    again: the frame records and the posterior particles are equal."""
    recs = []
    other = make_engine("B")
    try:
        for refine in (True, False):
            eng, st = stepped_engine("A", 2048, pf.STATE_F32, seed=11)
            try:
                if refine:
                    pa, ra, ba = hyps("A", 65)
                    pb, rb, bb = hyps("B", 3)
                    lead = pf.Engine.refine_multi([eng, other], [pa, pb], [ra, rb], [ba, bb], want_cov=True)
                    memb = pf.Engine.refine_multi([other, eng], [pb, pa], [rb, ra], [bb, ba], want_cov=True)
                    same(lead, memb[::-1])
                    same(lead, singles([eng, other], [pa, pb], [ra, rb], [ba, bb]))
                fr = st.frames[1]
                out = eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs,
                                              dt=fr.dt, seed=12, frame_idx=1))
                recs.append((bytes(out), eng.get_particles(1).tobytes()))
            finally:
                eng.close()
    finally:
        other.close()
    assert recs[0] == recs[1]


# ------------------------------------------------------------------------------------------------- closed loop
def test_closed_loop_four_objects():
    """4 objects stepped as one batch for 3 frames; after each frame the winners of the accepted streams are refined
    as one batch (K = 0 for the others) and equal the per-object refine_poses."""
    S, n_frames, N = 4, 3, 1000
    streams = [syn.make_stream(syn.StreamConfig(f"o{s}", M=5, B=20, N=N, seed=s), n_frames, t0=0.5 + 0.1 * s)
               for s in range(S)]
    engs = []
    for st in streams:
        e = pf.Engine(device=0, max_particles=N, state_dtype=pf.STATE_F32)
        e.set_model(st.markers, st.K)
        e.set_prior(st.prior(N))
        engs.append(e)
    accepted = 0
    try:
        for f in range(n_frames):
            frs = [st.frames[f] for st in streams]
            ins = [engs[s].make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                      seed=400 + 7 * s + f, frame_idx=f) for s, fr in enumerate(frs)]
            outs = pf.Engine.step_multi(engs, ins)
            poses, pairs = [], []
            for o in outs:
                ok = o.flag_fail == pf.FLAG_ACCEPTED
                accepted += int(ok)
                poses.append(np.array(o.winner_pose).reshape(1, 12) if ok else np.zeros((0, 12)))
                pairs.append(np.array(o.corr, dtype=np.uint32).reshape(1, pf.MAX_MARKERS, 2) if ok
                             else np.zeros((0, pf.MAX_MARKERS, 2), dtype=np.uint32))
            blobs = [fr.blobs for fr in frs]
            got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
            same(got, singles(engs, poses, pairs, blobs), f)
            for s, o in enumerate(outs):
                if len(poses[s]):
                    assert got[s]["best"] == 0 and got[s]["rows"]["n_pairs"][0] == o.n_corr, (f, s)
    finally:
        close_all(engs)
    assert accepted >= S  # the loop refined something


# ------------------------------------------------------------------------------------------------------ errors
class RawBatch:
    """The C arrays of a pfmpe_refine_multi call, with out / rows / cov prefilled with a byte pattern."""
    PATTERN = 0xA5

    def __init__(self, engs, poses, pairs, blobs):
        S = self.S = len(engs)
        self.engs = engs
        self.ctxs = (C.c_void_p * S)(*[e.ctx.value if e is not None else None for e in engs])
        self.ins, self.outs = (pf.RefineIn * S)(), (pf.RefineOut * S)()
        self.params = (pf.RefineParams * S)()
        self.keep, self.rows, self.covs = [], [], []
        for s in range(S):
            ai, kb = pf.Engine._assoc_in(blobs[s], -1)
            po = np.ascontiguousarray(poses[s], dtype=np.float64).reshape(-1, 12)
            pr = np.ascontiguousarray(pairs[s], dtype=np.uint32).reshape(-1, pf.MAX_MARKERS, 2)
            self.keep.append([kb, po, pr])
            self.ins[s].blobs, self.ins[s].K = ai, len(po)
            self.ins[s].poses, self.ins[s].corr = po.ctypes.data_as(DP), pr.ctypes.data_as(U32)
            pf.load().pfmpe_default_refine_params(C.byref(self.params[s]))
            self.rows.append(np.zeros(max(len(po), 1), dtype=pf.REFINE_ROW_DTYPE))
            self.covs.append(np.zeros((max(len(po), 1), 36)))
        self.rp = (C.c_void_p * S)(*[r.ctypes.data for r in self.rows])
        self.cp = (DP * S)(*[c.ctypes.data_as(DP) for c in self.covs])
        self.prefill()

    def prefill(self):
        C.memset(self.outs, self.PATTERN, C.sizeof(self.outs))
        for a in self.rows + self.covs:
            a.view(np.uint8).reshape(-1)[:] = self.PATTERN

    def untouched(self):
        return (bytes(self.outs) == bytes([self.PATTERN]) * C.sizeof(self.outs)
                and all((a.view(np.uint8) == self.PATTERN).all() for a in self.rows + self.covs))

    def call(self, S=None, ctxs="own", ins="own", outs="own", params=None):
        return pf.load().pfmpe_refine_multi(self.ctxs if ctxs == "own" else ctxs, self.S if S is None else S,
                                            self.ins if ins == "own" else ins, params,
                                            self.outs if outs == "own" else outs, self.rp, self.cp)


def test_errors():
    names = ("A", "B", "C")
    engs = [make_engine(n) for n in names]
    small = make_engine("A", max_particles=8, max_blobs=32)
    bare = make_engine("A", model=False)
    big = [make_engine("A", max_particles=65536), make_engine("B", max_particles=65536)]
    try:
        poses, pairs, blobs = map(list, zip(*[hyps(n, 4) for n in names]))
        M = [len(rr.cloud(n)[0]) for n in names]
        ref = singles(engs, poses, pairs, blobs)

        def fresh(e=engs, po=poses, pr=pairs, bl=blobs):
            return RawBatch(list(e), po, pr, bl)

        def refused(rb, rc, code, stream, **kw):
            assert rc == code, (rc, code, stream, kw)
            assert rb.untouched(), (code, stream)
            if stream is not None:
                text = rb.engs[0].last_error()
                assert text.startswith(f"refine_multi: stream {stream}: "), text

        def mutated(fn, code, stream, e=engs, po=poses, pr=pairs, bl=blobs, **kw):
            rb = fresh(e, po, pr, bl)
            fn(rb)
            refused(rb, rb.call(**kw), code, stream)

        # no context to report on
        rb = fresh()
        refused(rb, rb.call(ctxs=None), pf.E_ARG, None)
        refused(rb, rb.call(S=0), pf.E_ARG, None)
        refused(rb, rb.call(S=-1), pf.E_ARG, None)
        null0 = fresh([None] + engs[1:])
        assert null0.call() == pf.E_ARG and null0.untouched()
        # the batch as a whole
        for kw in ({"ins": None}, {"outs": None}):
            assert rb.call(**kw) == pf.E_ARG and rb.untouched()
            assert engs[0].last_error().startswith("refine_multi: ")
        many = RawBatch([engs[s % 3] for s in range(65)], [poses[s % 3] for s in range(65)],
                        [pairs[s % 3] for s in range(65)], [blobs[s % 3] for s in range(65)])
        assert many.call() == pf.E_CAP and many.untouched()
        assert many.call(S=64) == pf.OK  # 64 streams are accepted
        # arguments of one stream
        rb = fresh([engs[0], None, engs[2]])
        refused(rb, rb.call(), pf.E_ARG, 1)
        mutated(lambda b: setattr(b.ins[1], "K", -1), pf.E_ARG, 1)
        mutated(lambda b: setattr(b.ins[2], "poses", DP()), pf.E_ARG, 2)
        mutated(lambda b: setattr(b.ins[0], "corr", U32()), pf.E_ARG, 0)
        mutated(lambda b: setattr(b.ins[1].blobs, "B", -1), pf.E_ARG, 1)
        mutated(lambda b: setattr(b.ins[2].blobs, "blobs", DP()), pf.E_ARG, 2)
        mutated(lambda b: setattr(b.ins[1].blobs, "bank_frame", 0), pf.E_ARG, 1)  # no bank staged
        bad = [p.copy() for p in pairs]
        bad[2][1, 0, 0] = M[2] + 1  # an LED index above M
        mutated(lambda b: None, pf.E_ARG, 2, pr=bad)
        bad = [p.copy() for p in pairs]
        bad[0][3, 1, 1] = len(blobs[0]) + 1  # a blob index above B
        mutated(lambda b: None, pf.E_ARG, 0, pr=bad)
        bad = [p.copy() for p in pairs]
        bad[1][0, 0] = (0, 1)  # LED 0 beside a blob
        mutated(lambda b: None, pf.E_ARG, 1, pr=bad)
        nan = [p.copy() for p in poses]
        nan[1][2, 7] = np.nan
        mutated(lambda b: None, pf.E_ARG, 1, po=nan)
        inf = [p.copy() for p in poses]
        inf[2][0, 3] = np.inf
        mutated(lambda b: None, pf.E_ARG, 2, po=inf)
        for field, value, stream in (("max_iter", 0, 1), ("max_iter", 10001, 2), ("converged", -1.0, 0),
                                     ("converged", float("nan"), 1)):
            rb = fresh()
            setattr(rb.params[stream], field, value)
            refused(rb, rb.call(params=rb.params), pf.E_ARG, stream)
        # capacity
        trio = [engs[0], small, engs[2]]
        mutated(lambda b: None, pf.E_CAP, 1, e=trio, bl=[blobs[0], np.zeros((33, 2)), blobs[2]])  # B > max_blobs
        p9, r9, _ = hyps("A", 9)
        mutated(lambda b: None, pf.E_CAP, 1, e=trio, po=[poses[0], p9, poses[2]], pr=[pairs[0], r9, pairs[2]],
                bl=[blobs[0], blobs[0], blobs[2]])  # K > max_particles
        zp = np.zeros((65536, 12))
        zr = np.zeros((65536, pf.MAX_MARKERS, 2), dtype=np.uint32)
        rb = RawBatch(big, [zp, zp[:1]], [zr, zr[:1]], [blobs[0], blobs[1]])  # 65,537 hypotheses in all
        refused(rb, rb.call(), pf.E_CAP, 1)
        # state
        mutated(lambda b: None, pf.E_STATE, 2, e=[engs[0], engs[1], bare], bl=[blobs[0], blobs[1], blobs[0]],
                po=[poses[0], poses[1], poses[0]], pr=[pairs[0], pairs[1], pairs[0]])
        # a K = 0 stream needs no poses or rows, but its other arguments are checked all the same
        rb = fresh(po=[poses[0], poses[1][:0], poses[2]], pr=[pairs[0], pairs[1][:0], pairs[2]])
        rb.ins[1].poses, rb.ins[1].corr = DP(), U32()
        rb.ins[1].blobs.B = -1
        refused(rb, rb.call(), pf.E_ARG, 1)
        # the binding raises with the code and the text
        with pytest.raises(pf.PFError) as e:
            pf.Engine.refine_multi(engs, nan, pairs, blobs)
        assert e.value.code == pf.E_ARG and "refine_multi: stream 1: " in str(e.value)
        # a valid call right after is still correct
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, want_cov=True)
        same(got, ref, "after the errors")
        rb = fresh()
        assert rb.call() == pf.OK and not rb.untouched()
        for s in range(3):
            assert rb.rows[s].tobytes() == ref[s]["rows"].tobytes()
            assert rb.covs[s].tobytes() == ref[s]["cov"].tobytes()
    finally:
        close_all(engs + [small, bare] + big)
