"""pfmpe_assoc_stats_multi on the device: every entry of a batch against the single call pfmpe_assoc_stats on the same
engine.  Everything is integers, so every comparison is exact: each field of the record and the whole votes table.
Shapes are small; the ones that can tell a wrong block-to-entry map or a wrong bins offset are the block seams
(N = 1, 255, 256, 257 in one batch, an entry with its own grid stride beside a one-particle entry) and the batch
that mixes the LDS and the direct voting path."""
import ctypes

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from pf_monocular_pose_estimator_amd import _capi
from test_gpu_parity import make_engine
from test_gpu_assoc import _stream, _frame, _stepped, _hist, markers_16

pytestmark = pytest.mark.gpu

STATES = [pf.STATE_F64, pf.STATE_F32, pf.STATE_F16]
PROP, POST = pf.ASSOC_PROPAGATED, pf.ASSOC_POSTERIOR
MM = pf.MAX_MARKERS


def _same(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def _check_batch(engines, whichs, blobs_list=None, bank_frames=None, what=""):
    """One batch against the single calls, entry by entry; returns the batch's dicts."""
    S = len(engines)
    got = pf.Engine.assoc_stats_multi(engines, whichs, blobs_list, bank_frames)
    assert len(got) == S
    for s in range(S):
        want = engines[s].assoc_stats(whichs[s], blobs=None if blobs_list is None else blobs_list[s],
                                      bank_frame=-1 if bank_frames is None else bank_frames[s])
        _same(got[s], want, (what, s))
        assert got[s]["n"] == engines[s].N and got[s]["M"] == engines[s].M
    return got


def _close(engines):
    for e in set(engines):
        e.close()


# ---- 1. three marker buckets in one batch
@pytest.mark.parametrize("state", STATES)
def test_three_buckets_both_sets(state):
    shapes = [(5, 50, 1000), (4, 3, 257), (12, 200, 1000)]
    made = [_stepped(M, B, N, state) for M, B, N in shapes]
    engines = [m[0] for m in made]
    blobs = [m[3] for m in made]
    try:
        for which in (PROP, POST):
            got = _check_batch(engines, [which] * 3, blobs, what=which)
            assert [(g["M"], g["B"]) for g in got] == [(5, 50), (4, 3), (12, 200)]
            assert all(g["n_any"] > 0 for g in got)  # the inputs do pair: the tables are not empty
        # both sets of every object in one batch: two set kinds x three buckets, six launches
        _check_batch(engines * 2, [PROP] * 3 + [POST] * 3, blobs * 2, what="both")
    finally:
        _close(engines)


# ---- 2. block seams
def test_block_seams_in_one_batch():
    Ns = [1, 255, 256, 257]
    made = [_stepped(5, 50, N, pf.STATE_F32) for N in Ns]
    engines = [m[0] for m in made]
    blobs = [m[3] for m in made]
    try:
        for which in (PROP, POST):
            got = _check_batch(engines, [which] * 4, blobs, what=which)
            assert [g["n"] for g in got] == Ns
        order = [3, 0, 2, 1]
        _check_batch([engines[i] for i in order], [POST] * 4, [blobs[i] for i in order], what="permuted")
    finally:
        _close(engines)


def test_grid_stride_entry_next_to_one_particle():
    """N = 1024 * 256 + 37: the entry's 1024 blocks walk a second round of 37 particles with the entry's own stride,
    next to an entry of one particle, in both orders."""
    big = _stepped(5, 50, 1024 * 256 + 37, pf.STATE_F16, fused=0)
    one = _stepped(5, 50, 1, pf.STATE_F16)
    engines = [big[0], one[0]]
    blobs = [big[3], one[3]]
    try:
        for order in ([0, 1], [1, 0]):
            got = _check_batch([engines[i] for i in order], [POST] * 2, [blobs[i] for i in order], what=order)
            assert sorted(g["n"] for g in got) == [1, 1024 * 256 + 37]
        _check_batch(engines, [PROP, PROP], blobs, what="propagated")
    finally:
        _close(engines)


# ---- 3. the LDS and the direct voting path in one batch
def _large_table_engine():
    """M = 16, B = 1024, as tests/test_gpu_assoc.py test_direct_votes_large_table builds it: the bins do not fit in LDS."""
    st = _stream(12, 200, 1000)
    fr = st.frames[0]
    mk = markers_16()
    rng = np.random.default_rng(3)
    true_px = syn.project(st.K, syn.to44(fr.current_pose), mk)
    near = true_px[rng.integers(0, 16, 400)] + rng.integers(1, 6, (400, 2)) * rng.choice([-1, 1], (400, 2))
    far = rng.uniform([0, 0], [syn.IMAGE_W, syn.IMAGE_H], size=(1024 - 16 - 400, 2))
    blobs = np.vstack([true_px, near, far])
    rng.shuffle(blobs)
    blobs = blobs.astype(np.float32).astype(np.float64)
    eng = pf.Engine(device=0, max_particles=1000, max_blobs=1024, state_dtype=pf.STATE_F32)
    eng.set_model(mk, st.K)
    eng.set_params(pf.default_params())
    eng.set_prior(st.prior(fast=True)[:1000])
    return eng, blobs


def test_direct_and_lds_entries_in_one_batch():
    large, lblobs = _large_table_engine()
    small, _, _, sblobs, _ = _stepped(5, 50, 1000, pf.STATE_F32)
    try:
        plan, _ = pf.host_assoc_plan([1000, 1000], [16, 5], [1024, 50])
        assert [p["lds_votes"] for p in plan] == [0, 1]
        for engines, blobs in (([large, small], [lblobs, sblobs]), ([small, large, small], [sblobs, lblobs, sblobs])):
            got = _check_batch(engines, [POST] * len(engines), blobs)
            for g, e, b in zip(got, engines, blobs):
                corr, n_corr = e.get_pairs(POST, blobs=b)
                votes, hist = _hist(corr, n_corr, e.M, len(b))
                assert np.array_equal(g["votes"], votes) and np.array_equal(g["npairs_hist"], hist)
                assert g["n_any"] > 0
        # the 5 x 50 context forced onto the direct path: the same tables
        lds = pf.Engine.assoc_stats_multi([small, large], [POST, POST], [sblobs, lblobs])
        small.set_option(pf.OPT_DIAG, pf.DIAG_ASSOC_DIRECT)
        direct = pf.Engine.assoc_stats_multi([small, large], [POST, POST], [sblobs, lblobs])
        both = pf.Engine.assoc_stats_multi([small, small], [PROP, POST], [sblobs, sblobs])
        small.set_option(pf.OPT_DIAG, 0)
        for s in range(2):
            _same(lds[s], direct[s], ("direct", s))
        _same(both[0], small.assoc_stats(PROP, blobs=sblobs), "direct propagated")
        _same(both[1], lds[0], "direct posterior")
    finally:
        _close([large, small])


# ---- 4. one context in four entries
def test_one_context_in_four_entries_and_no_blobs():
    eng, st, mk, blobs, _ = _stepped(5, 50, 1000, pf.STATE_F32)
    other = blobs[::-1][:31].copy()  # a second list: other indices, another B
    none = np.zeros((0, 2))
    try:
        whichs = [PROP, POST, PROP, POST, POST, PROP]
        lists = [blobs, blobs, other, other, none, none]
        got = _check_batch([eng] * 6, whichs, lists)
        for g, which, bl in zip(got, whichs, lists):
            corr, n_corr = eng.get_pairs(which, blobs=bl)
            votes, hist = _hist(corr, n_corr, 5, len(bl))
            assert g["votes"].shape == (5, len(bl) + 1)
            assert np.array_equal(g["votes"], votes) and np.array_equal(g["npairs_hist"], hist)
        assert got[4]["B"] == 0 and np.all(got[4]["votes"] == 1000) and got[4]["n_any"] == 0
        assert got[0]["n_any"] > 0 and got[2]["n_any"] > 0
        # the table is not wanted: the records alone
        bare = pf.Engine.assoc_stats_multi([eng] * 2, [PROP, POST], [blobs, other], want_votes=False)
        for b, g in zip(bare, (got[0], got[3])):
            assert "votes" not in b
            _same(b, {k: v for k, v in g.items() if k != "votes"})
    finally:
        eng.close()


# ---- 5. bank frames
def test_bank_frames_of_each_context():
    a, _, _, ablobs, _ = _stepped(5, 50, 1000, pf.STATE_F32)
    b, _, _, bblobs, _ = _stepped(12, 200, 700, pf.STATE_F32)
    try:
        a.stage_blob_bank([np.zeros((3, 2)), ablobs, ablobs[:17]])
        b.stage_blob_bank([bblobs, np.zeros((0, 2))])
        got = pf.Engine.assoc_stats_multi([a, b, a, b], [POST, PROP, PROP, POST], bank_frames=[1, 0, 2, 1])
        assert [g["B"] for g in got] == [50, 200, 17, 0]
        _same(got[0], a.assoc_stats(POST, blobs=ablobs))
        _same(got[1], b.assoc_stats(PROP, blobs=bblobs))
        _same(got[2], a.assoc_stats(PROP, blobs=ablobs[:17]))
        _same(got[3], b.assoc_stats(POST, blobs=np.zeros((0, 2))))
        # a bank frame and a host list in one batch
        mix = pf.Engine.assoc_stats_multi([a, b], [POST, POST], [None, bblobs], [2, -1])
        _same(mix[0], a.assoc_stats(POST, bank_frame=2))
        _same(mix[1], b.assoc_stats(POST, blobs=bblobs))
    finally:
        _close([a, b])


# ---- 6. mixed pruning options
def test_mixed_pruning_options():
    made = [_stepped(5, 50, 1000, pf.STATE_F32) for _ in range(2)]
    engines = [m[0] for m in made]
    blobs = [m[3] for m in made]
    try:
        engines[1].set_option(pf.OPT_PRUNE, 0)
        plan, total = pf.host_assoc_plan([1000, 1000], [5, 5], [50, 50], prune=[1, 0])
        assert total["launches"] == 2
        for which in (PROP, POST):
            got = _check_batch(engines, [which] * 2, blobs, what=which)
            _same(got[0], got[1], "pruning changes no pair")  # the two engines took the same step
    finally:
        _close(engines)


# ---- 7. scratch reuse
def _raw_multi(engines, whichs, blobs_list, S=None, fill=None, votes_null=False):
    """The C call itself: (code, the S records as bytes, the votes tables as arrays)."""
    n = len(engines)
    S = n if S is None else S
    ctxs = (ctypes.c_void_p * max(n, 1))(*[e.ctx.value if e is not None else None for e in engines])
    ins = (_capi.AssocMultiIn * max(n, 1))()
    keep, tabs = [], []
    vps = (ctypes.POINTER(ctypes.c_uint32) * max(n, 1))()
    for s in range(n):
        bl = np.ascontiguousarray(blobs_list[s], dtype=np.float64).reshape(-1, 2)
        keep.append(bl)
        ins[s].blobs.blobs = bl.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ins[s].blobs.B = len(bl)
        ins[s].blobs.bank_frame = -1
        ins[s].which = whichs[s]
        M = (engines[s].M if engines[s] is not None else 0) or MM  # (no context or no model: room for any)
        tabs.append(np.full(M * (len(bl) + 1), 0xABABABAB, dtype=np.uint32))
        vps[s] = tabs[s].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    if fill is not None:
        fill(ins)
    outs = (_capi.AssocOut * max(n, 1))()
    ctypes.memset(outs, 0xAB, ctypes.sizeof(outs))
    rc = pf.load().pfmpe_assoc_stats_multi(ctxs, S, ins, outs, None if votes_null else vps)
    return rc, bytes(outs), tabs


def test_scratch_reuse_large_small_large():
    large = [_stepped(12, 200, 1000, pf.STATE_F32) for _ in range(2)] + [_stepped(5, 50, 1000, pf.STATE_F32)]
    engines = [m[0] for m in large]
    blobs = [m[3] for m in large]
    try:
        big = (engines * 3, [POST] * 9, blobs * 3)
        small = ([engines[2]], [POST], [blobs[2][:7]])
        first = None
        for args in (big, small, big):
            _check_batch(*args)
            rc, rec, tabs = _raw_multi(*args)
            rc2, rec2, tabs2 = _raw_multi(*args)
            assert rc == pf.OK and rc2 == pf.OK and rec == rec2
            assert all(np.array_equal(x, y) for x, y in zip(tabs, tabs2))
            if args is big:
                if first is None:
                    first = (rec, tabs)
                else:
                    assert rec == first[0] and all(np.array_equal(x, y) for x, y in zip(tabs, first[1]))
    finally:
        _close(engines)


# ---- 8. reads only
def test_batch_reads_only():
    N = 1000
    st = _stream(5, 50, N, 2)

    def fresh(seed_shift):
        e = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
        e.set_prior(st.prior(fast=True) if not seed_shift else st.prior(fast=True)[::-1].copy())
        return e

    batch, twins = [fresh(0), fresh(1)], [fresh(0), fresh(1)]
    try:
        for s in range(2):
            for e in (batch[s], twins[s]):
                e.step(_frame(e, st.frames[0], 0))
        before = [(e.get_particles(1), e.get_weights(), e.get_particles(0)) for e in batch]
        got = pf.Engine.assoc_stats_multi(batch * 2, [PROP, PROP, POST, POST], [st.frames[0].blobs] * 4)
        assert all(g["n_any"] > 0 for g in got)
        for e, (p1, w, p0) in zip(batch, before):
            assert np.array_equal(e.get_particles(1), p1) and np.array_equal(e.get_weights(), w)
            assert np.array_equal(e.get_particles(0), p0)
        for s in range(2):
            a = batch[s].step(_frame(batch[s], st.frames[1], 1))
            b = twins[s].step(_frame(twins[s], st.frames[1], 1))
            for k, v in a.as_dict().items():
                assert np.array_equal(np.asarray(v), np.asarray(b.as_dict()[k])), (s, k)
            assert np.array_equal(batch[s].get_particles(1), twins[s].get_particles(1))
            assert np.array_equal(batch[s].get_weights(), twins[s].get_weights())
    finally:
        _close(batch + twins)


# ---- 9. ordering after the members' own streams
def test_ordered_after_members_own_steps():
    N = 1000
    st = _stream(5, 50, N, 3)
    engines = []
    try:
        for s in range(4):
            e = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX, fused=0 if s % 2 else 2)
            e.set_prior(st.prior(fast=True) if s < 2 else st.prior(fast=True)[::-1].copy())
            engines.append(e)
        blobs = None
        for f in range(3):
            for e in engines:  # S single steps on the members' own streams, then the batch at once
                e.step(_frame(e, st.frames[f], f))
            blobs = [st.frames[f].blobs] * 4
            got_prop = pf.Engine.assoc_stats_multi(engines, [PROP] * 4, blobs)
            got_post = pf.Engine.assoc_stats_multi(engines[::-1], [POST] * 4, blobs)  # another leader
            for s, e in enumerate(engines):
                _same(got_prop[s], e.assoc_stats(PROP, blobs=blobs[s]), (f, s))
                _same(got_post[3 - s], e.assoc_stats(POST, blobs=blobs[s]), (f, s))
    finally:
        _close(engines)


# ---- 10. errors
# (Two of the listed errors have no input here: a device mismatch needs two devices, and no table build_table can
# produce exceeds the LDS, the largest being 63,584 bytes; tests/test_assoc_multi_host.py reaches that code through
# the plan's table sizes.)
def test_errors_leave_outputs_untouched():
    st = _stream(5, 50, 1000)
    fr = st.frames[0]
    blobs = fr.blobs
    good, _, _, gblobs, _ = _stepped(5, 50, 1000, pf.STATE_F32)
    other_state, _, _, _, _ = _stepped(5, 50, 1000, pf.STATE_F64)
    bare = pf.Engine(device=0, max_particles=1000, max_blobs=64, state_dtype=pf.STATE_F32)
    lib = pf.load()

    def untouched(rec, tabs):
        return rec == b"\xab" * len(rec) and all(np.all(t == 0xABABABAB) for t in tabs)

    def expect(code, engines, whichs, lists, at=None, text=None, **kw):
        rc, rec, tabs = _raw_multi(engines, whichs, lists, **kw)
        assert rc == code, (rc, good.last_error())
        assert untouched(rec, tabs)
        if at is not None:
            msg = good.last_error()
            assert msg.startswith("assoc_stats_multi: stream %d: " % at), msg
            if text:
                assert text in msg, msg

    try:
        # no model / no particle set / no step yet, each in the second entry
        expect(pf.E_STATE, [good, bare], [POST, POST], [gblobs, blobs], at=1)
        bare.set_model(st.markers, st.K)
        expect(pf.E_STATE, [good, bare], [POST, POST], [gblobs, blobs], at=1)
        bare.set_prior(st.prior(fast=True))
        expect(pf.E_STATE, [good, good, bare], [POST, PROP, PROP], [gblobs, gblobs, blobs], at=2, text="no step yet")
        assert _raw_multi([good, bare], [PROP, POST], [gblobs, blobs])[0] == pf.OK
        # arguments
        expect(pf.E_ARG, [good, good], [POST, 2], [gblobs, gblobs], at=1, text="bad which")
        expect(pf.E_ARG, [good, good], [-1, POST], [gblobs, gblobs], at=0, text="bad which")
        expect(pf.E_ARG, [good, other_state], [POST, POST], [gblobs, gblobs], at=1, text="state type")
        expect(pf.E_ARG, [good, None], [POST, POST], [gblobs, gblobs], at=1, text="null context")

        def neg_b(ins):
            ins[1].blobs.B = -1

        def null_blobs(ins):
            ins[1].blobs.blobs = ctypes.POINTER(ctypes.c_double)()

        def no_bank(ins):
            ins[1].blobs.bank_frame = 0

        def far_bank(ins):
            ins[0].blobs.bank_frame = 5

        expect(pf.E_ARG, [good, good], [POST, POST], [gblobs, gblobs], at=1, text="B < 0", fill=neg_b)
        expect(pf.E_ARG, [good, good], [POST, POST], [gblobs, gblobs], at=1, text="null blobs", fill=null_blobs)
        expect(pf.E_ARG, [good, good], [POST, POST], [gblobs, gblobs], at=1, text="bank_frame", fill=no_bank)
        good.stage_blob_bank([gblobs, gblobs[:9]])
        expect(pf.E_ARG, [good, good], [POST, POST], [gblobs, gblobs], at=0, text="bank_frame", fill=far_bank)
        # S < 1, NULL pointers
        rc, rec, tabs = _raw_multi([good], [POST], [gblobs], S=0)
        assert rc == pf.E_ARG and untouched(rec, tabs)
        rc, rec, tabs = _raw_multi([None, good], [POST, POST], [gblobs, gblobs])
        assert rc == pf.E_ARG and untouched(rec, tabs)
        ctxs = (ctypes.c_void_p * 1)(good.ctx.value)
        ins = (_capi.AssocMultiIn * 1)()
        ins[0].blobs.bank_frame = -1
        ins[0].which = POST
        outs = (_capi.AssocOut * 1)()
        assert lib.pfmpe_assoc_stats_multi(None, 1, ins, outs, None) == pf.E_ARG
        assert lib.pfmpe_assoc_stats_multi(ctxs, 1, None, outs, None) == pf.E_ARG
        assert lib.pfmpe_assoc_stats_multi(ctxs, 1, ins, None, None) == pf.E_ARG
        # capacity: S = 65, an entry's B above its context's max_blobs
        expect(pf.E_CAP, [good] * 65, [POST] * 65, [gblobs[:2]] * 65)
        assert "PFMPE_ASSOC_MAX_STREAMS" in good.last_error()
        bare.step(_frame(bare, fr))
        expect(pf.E_CAP, [good, bare], [POST, POST], [gblobs, np.zeros((65, 2))], at=1, text="max_blobs")
        # S = 64 is a batch, votes = NULL is allowed, and the contexts still work
        rc, rec, tabs = _raw_multi([good] * 64, [POST, PROP] * 32, [gblobs] * 64)
        assert rc == pf.OK
        want = good.assoc_stats(PROP, blobs=gblobs)
        assert np.array_equal(tabs[63].reshape(5, 51), want["votes"])
        rc, rec, tabs = _raw_multi([good, bare], [POST, PROP], [gblobs, blobs], votes_null=True)
        assert rc == pf.OK and all(np.all(t == 0xABABABAB) for t in tabs)
        _check_batch([good, bare], [PROP, POST], [gblobs, blobs])
    finally:
        _close([good, other_state, bare])


# ---- 11. the gated frame end to end
def _decoyed(st, fr, led):
    """The frame's blobs plus two decoys 1.5 px either side of one LED's true projection."""
    px = syn.project(st.K, fr.truth, st.markers)[led]
    extra = np.array([px + [1.5, 0.0], px - [1.5, 0.0]])
    return np.vstack([fr.blobs, extra]).astype(np.float32).astype(np.float64)


def test_gated_frame_batch_equals_single_chain():
    N = 1000
    st = _stream(5, 50, N, 1)
    fr = st.frames[0]
    lists = [_decoyed(st, fr, 1), fr.blobs, _decoyed(st, fr, 3)]

    def fresh(s):
        e = make_engine(N, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
        e.set_prior(st.prior(fast=True) if s != 1 else st.prior(fast=True)[::-1].copy())
        return e

    batch, singles = [fresh(s) for s in range(3)], [fresh(s) for s in range(3)]
    try:
        # the batch form: three calls after detection
        outs = pf.Engine.step_multi(batch, [_frame(batch[s], fr, 0, blobs=lists[s]) for s in range(3)])
        stats = pf.Engine.assoc_stats_multi(batch, [POST] * 3, lists)
        gates = [pf.host_gate_pairs(stats[s]["votes"], outs[s].pairs()) for s in range(3)]
        starts = [np.array(o.winner_pose if o.resampled else o.most_likely_pose) for o in outs]
        refined = pf.Engine.refine_multi(batch, [p[None] for p in starts], [g["gated"][None] for g in gates], lists)
        # the per-object chain of single calls
        for s, e in enumerate(singles):
            o = e.step(_frame(e, fr, 0, blobs=lists[s]))
            assert np.array_equal(o.pairs(), outs[s].pairs())
            a = e.assoc_stats(POST, blobs=lists[s])
            _same(stats[s], a, s)
            g = pf.host_gate_pairs(a["votes"], o.pairs())
            for k in g:
                assert np.array_equal(np.asarray(g[k]), np.asarray(gates[s][k])), (s, k)
            start = np.array(o.winner_pose if o.resampled else o.most_likely_pose)
            r = e.refine_poses(start[None], g["gated"][None], blobs=lists[s])
            assert r["rows"].tobytes() == refined[s]["rows"].tobytes(), s
            for k in ("n", "n_with_pairs", "n_converged", "best"):
                assert r[k] == refined[s][k], (s, k)
        for s, g in enumerate(gates):
            print("object", s, "n_in", g["n_in"], "n_gated", g["n_gated"], "fallback", g["fallback"],
                  "reason", g["reason"].tolist())
        # the gate did something: some object's row lost a pair and still went to Gauss-Newton gated
        assert any(g["n_gated"] < g["n_in"] and not g["fallback"] for g in gates)
    finally:
        _close(batch + singles)
