"""pfmpe_top_particles on the device against numpy over the engine's own read-backs (get_weights, get_counts,
get_particles(0), get_pairs): the ranking (larger key first, lower index first among equal keys, key > 0 only), the
rows that go with it, the suppression walk against pfmpe_host_top_suppress, and the identities that tie the call to
the frame record and to the refinement.  Everything is integers or copied doubles: every comparison is exact.

The suppression cases assert the condition of tests/test_top_host.py on their inputs: no pair of the pool decides
within a relative 1e-9 of a threshold."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from pf_monocular_pose_estimator_amd import _capi
from test_gpu_parity import make_engine
from test_top_host import assert_margin

pytestmark = pytest.mark.gpu

STATES = [pf.STATE_F64, pf.STATE_F32, pf.STATE_F16]
KEYS = [pf.TOP_BY_WEIGHT, pf.TOP_BY_COUNT]
MM = pf.MAX_MARKERS
CAP = pf.TOP_MAX
SENT_I, SENT_F, SENT_U = -12345, -7.25, 0xDEADBEEF


@functools.lru_cache(maxsize=None)
def _stream(M, B, N, n_frames):
    return syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=N), n_frames)


def _frame(eng, fr, f=0, blobs=None, **kw):
    return eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs if blobs is None else blobs,
                          dt=fr.dt, seed=900 + f, frame_idx=f, **kw)


def _stepped(N, state, fused=2, blobs=None, n_frames=1):
    """An engine after one step of the (M = 5, B = 50, N) stream, with the frame's blobs and its record."""
    st = _stream(5, 50, max(N, 1000), n_frames)
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX, fused=fused)
    eng.set_prior(st.prior(fast=True)[:N])
    fr = st.frames[0]
    out = eng.step(_frame(eng, fr, blobs=blobs))
    return eng, st, fr.blobs, out


class Raw:
    """One C call with a sentinel in every slot of every output array."""

    def __init__(self, eng, key, K, min_trans=0.0, min_rot=0.0, blobs=None, ai=None, null=(), ctx=True):
        self.index = np.full(CAP, SENT_I, dtype=np.int32)
        self.key_value = np.full(CAP, SENT_F, dtype=np.float64)
        self.poses = np.full((CAP, 12), SENT_F, dtype=np.float64)
        self.corr = np.full((CAP, MM, 2), SENT_U, dtype=np.uint32)
        self.n_corr = np.full(CAP, SENT_I, dtype=np.int32)
        self.out = _capi.TopOut(-1, -2, -3, -4)
        prm = _capi.TopParams(int(key), int(K), float(min_trans), float(min_rot))
        keep = None
        if ai is None and blobs is not None:
            ai, keep = eng._assoc_in(blobs, -1)
        ip, up = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        self.rc = eng.lib.pfmpe_top_particles(
            eng.ctx if ctx else None, None if "params" in null else C.byref(prm), C.byref(ai) if ai is not None else None,
            None if "out" in null else C.byref(self.out), self.index.ctypes.data_as(ip), _capi._dptr(self.key_value),
            _capi._dptr(self.poses), self.corr.ctypes.data_as(up), self.n_corr.ctypes.data_as(ip))

    def untouched(self, n=0, pairs=True):
        """Every slot from row n on still holds its sentinel (the pair rows from row 0 when no blobs were given)."""
        m = n if pairs else 0
        return bool(np.all(self.index[n:] == SENT_I) and np.all(self.key_value[n:] == SENT_F)
                    and np.all(self.poses[n:] == SENT_F) and np.all(self.corr[m:] == SENT_U)
                    and np.all(self.n_corr[m:] == SENT_I))

    def out_untouched(self):
        o = self.out
        return (o.n, o.n_positive, o.n_out, o.n_examined) == (-1, -2, -3, -4)

    def rows(self):
        n = self.out.n_out
        return (self.out.n, self.out.n_positive, n, self.out.n_examined, self.index[:n].tobytes(),
                self.key_value[:n].tobytes(), self.poses[:n].tobytes(), self.corr[:n].tobytes(), self.n_corr[:n].tobytes())


def _keys_of(eng, key):
    return eng.get_weights() if key == pf.TOP_BY_WEIGHT else eng.get_counts().astype(np.float64)


def _ranking(k):
    idx = np.arange(len(k))
    order = np.lexsort((idx, -k))
    return order[k[order] > 0]


def _check_ranking(eng, blobs, key, K, k, order, parts, corr, n_corr):
    r = Raw(eng, key, K, blobs=blobs)
    assert r.rc == pf.OK, eng.last_error()
    n_pos = len(order)
    n = min(K, n_pos)
    assert (r.out.n, r.out.n_positive, r.out.n_out, r.out.n_examined) == (len(k), n_pos, n, n)
    assert np.array_equal(r.index[:n], order[:n])
    assert np.array_equal(r.key_value[:n], k[order[:n]])
    assert r.poses[:n].tobytes() == parts[order[:n]].tobytes()
    assert np.array_equal(r.corr[:n], corr[order[:n]])
    assert np.array_equal(r.n_corr[:n], n_corr[order[:n]])
    assert r.untouched(n)
    return r


# ---- 1. the ranking and its rows: both keys, all three state types, one block .. strips beyond the grid
@pytest.mark.parametrize("state,N", [(s, n) for n in (1, 255, 1000, 70001, 300001) for s in STATES
                                     if not (n == 300001 and s == pf.STATE_F64)])  # 300,001: fp32 and fp16 state
def test_ranking(state, N):
    eng, st, blobs, out = _stepped(N, state, fused=0 if N == 300001 else 2)
    try:
        if N >= 255:
            assert out.resampled
        parts = eng.get_particles(0)
        corr, n_corr = eng.get_pairs(pf.ASSOC_PROPAGATED, blobs=blobs)
        for key in KEYS:
            if key == pf.TOP_BY_COUNT and not out.resampled:
                r = Raw(eng, key, 8, blobs=blobs)
                assert r.rc == pf.E_STATE and r.untouched() and r.out_untouched()
                continue
            k = _keys_of(eng, key)
            order = _ranking(k)
            print(f"state={state} N={N} key={key}: n_positive={len(order)}")
            for K in (0, 1, 8, 1024):
                _check_ranking(eng, blobs, key, K, k, order, parts, corr, n_corr)
            # without blobs: no pair row is written; the Python method returns the same rows
            r = Raw(eng, key, 8)
            n = min(8, len(order))
            assert r.rc == pf.OK and r.out.n_out == n and np.array_equal(r.index[:n], order[:n])
            assert r.untouched(n, pairs=False)
            d = eng.top_particles(key=key, K=8, blobs=blobs)
            assert np.array_equal(d["index"], order[:n]) and d["poses"].tobytes() == parts[order[:n]].tobytes()
            assert np.array_equal(d["corr"], corr[order[:n]]) and (d["n"], d["n_positive"]) == (N, len(order))
    finally:
        eng.close()


# ---- 2. ties
@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F64])
def test_count_ties_take_the_lowest_indices(state):
    """Resample counts of 1 and 2 come by the thousand: the threshold class has more members than are taken."""
    eng, st, blobs, out = _stepped(70001, state)
    try:
        assert out.resampled
        k = eng.get_counts().astype(np.float64)
        order = _ranking(k)
        for K in (64, 1024):
            assert len(order) > K
            thr = k[order[K - 1]]
            members, taken = int(np.sum(k == thr)), int(np.sum(k[order[:K]] == thr))
            print(f"K={K}: threshold count {thr}, {members} members, {taken} taken")
            if K == 1024:  # the pool's threshold class: the selection must take its lowest indices
                assert members > taken >= 1
            r = Raw(eng, pf.TOP_BY_COUNT, K)
            assert r.rc == pf.OK and r.out.n_out == K
            assert np.array_equal(r.index[:K], order[:K])
    finally:
        eng.close()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N", [1000, 70001])
def test_weight_ties_every_weight_equal(state, N):
    """Zero noise ranges and a prior of N identical poses (set_params accepts that): every particle is the same pose,
    every weight ties, and the rows are particles 0 .. K - 1."""
    st = _stream(5, 50, 1000, 1)
    prm = pf.default_params()
    prm.ang_min = prm.ang_max = prm.trans_min = prm.trans_max = 0.0
    eng = make_engine(N, st.markers, st.K, state, pf.RNG_PHILOX, params=prm)
    try:
        X = np.asarray(st.frames[0].current_pose, np.float64).astype(np.float32).astype(np.float64)
        eng.set_prior(np.tile(X, (N, 1)))
        blobs = syn.project(st.K, syn.to44(X), st.markers) + 0.25
        eye = np.eye(4)[:3].reshape(12)
        eng.step(eng.make_frame(X, X, eye, blobs=blobs, seed=5))
        w = eng.get_weights()
        assert np.unique(w).size == 1 and w[0] > 0, "the input does not tie every weight"
        for K in (1, 8, 1024):
            r = Raw(eng, pf.TOP_BY_WEIGHT, K)
            n = min(K, N)
            assert r.rc == pf.OK and (r.out.n_positive, r.out.n_out) == (N, n)
            assert np.array_equal(r.index[:n], np.arange(n))
            assert np.all(r.key_value[:n] == w[0]) and r.untouched(n, pairs=False)
    finally:
        eng.close()


# ---- 3. fewer eligible particles than rows wanted; no eligible particle at all
@pytest.mark.parametrize("state", STATES)
def test_K_above_n_positive(state):
    eng, st, blobs, out = _stepped(255, state)
    try:
        for key in KEYS:
            k = _keys_of(eng, key)
            order = _ranking(k)
            assert 0 < len(order) <= 255
            r = Raw(eng, key, 1024, blobs=blobs)
            assert r.rc == pf.OK and r.out.n_out == len(order) and r.out.n_positive == len(order)
            assert np.array_equal(r.index[: len(order)], order) and r.untouched(len(order))
    finally:
        eng.close()


@pytest.mark.parametrize("state", STATES)
def test_reinit_frame_has_no_eligible_particle(state):
    """B = 0: every weight is 0 and the step does not resample."""
    eng, st, blobs, out = _stepped(1000, state, blobs=np.zeros((0, 2)))
    try:
        assert not out.resampled and not np.any(eng.get_weights() > 0)
        r = Raw(eng, pf.TOP_BY_WEIGHT, 8, blobs=blobs, min_trans=0.002)
        assert r.rc == pf.OK
        assert (r.out.n, r.out.n_positive, r.out.n_out, r.out.n_examined) == (1000, 0, 0, 0) and r.untouched()
        r = Raw(eng, pf.TOP_BY_COUNT, 8)
        assert r.rc == pf.E_STATE and r.untouched() and r.out_untouched()
    finally:
        eng.close()


# ---- 4. the frame record
@pytest.mark.parametrize("state", STATES)
def test_frame_record_identities(state):
    eng, st, blobs, out = _stepped(1000, state)
    try:
        assert out.accepted and out.resampled
        r = Raw(eng, pf.TOP_BY_WEIGHT, 1, blobs=blobs)
        assert r.rc == pf.OK and r.out.n_out == 1
        assert r.index[0] == out.most_likely_idx
        assert np.array_equal(r.poses[0], np.array(out.most_likely_pose))
        assert r.key_value[0] == eng.get_weights().max()
        r = Raw(eng, pf.TOP_BY_COUNT, 1, blobs=blobs)
        assert r.rc == pf.OK and r.out.n_out == 1
        assert r.index[0] == out.winner_idx
        assert np.array_equal(r.poses[0], np.array(out.winner_pose))
        assert r.n_corr[0] == out.n_corr
        assert np.array_equal(r.corr[0].reshape(-1), np.array(out.corr, dtype=np.uint32))
    finally:
        eng.close()


# ---- 5. both frame shapes give the same bytes
@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F16])
def test_frame_shapes_agree(state):
    got = []
    for fused in (2, 0):
        eng, st, blobs, out = _stepped(70001, state, fused=fused)
        try:
            assert eng.info(pf.INFO_LAST_SHAPE) == (pf.SHAPE_FRAME2 if fused == 2 else pf.SHAPE_TWO_LAUNCH)
            rows = []
            for key in KEYS:
                for mt in (0.0, 0.002):
                    r = Raw(eng, key, 64, min_trans=mt, blobs=blobs)
                    assert r.rc == pf.OK
                    rows.append(r.rows())
            got.append(rows)
        finally:
            eng.close()
    assert got[0] == got[1]


# ---- 6. suppression: the device walk is the host walk on the pool's poses
# tr = 1 + 2 cos(angle) lies near 3 for every pair of a cloud, so a relative 1e-9 of it is a wide window in the angle:
# among the half million pairs of a full pool some pair sits inside it for every rotation threshold within the cloud's
# spread (pair angles up to 0.053 rad).  The full pool therefore takes a rotation threshold just outside the spread,
# and the thresholds that cut through a cloud run on the 78 .. 84 eligible particles of the N = 255 frame.
SUPPRESS = {"2mm": (0.002, 0.0), "10m": (10.0, 0.0), "rotation": (0.0, 0.05)}
SUPPRESS_SMALL = {"rotation 4 mrad": (0.0, 0.004), "rotation 13 mrad": (0.0, 0.013), "both": (0.002, 0.013)}


def _check_suppression(eng, state, key, blobs, cases):
    """Every case at K = 1, 8, 1024 against the host walk over the unsuppressed pool; returns {(case, K): n_out}."""
    pool = Raw(eng, key, 1024, blobs=blobs)
    assert pool.rc == pf.OK
    P = pool.out.n_out
    assert P == min(1024, pool.out.n_positive) and P > 64
    poses = pool.poses[:P]
    kept = {}
    for name, (mt, mr) in cases.items():
        assert_margin(poses, mt, mr)
        for K in (1, 8, 1024):
            want = pf.host_top_suppress(poses, K, mt, mr)
            r = Raw(eng, key, K, min_trans=mt, min_rot=mr, blobs=blobs)
            assert r.rc == pf.OK, eng.last_error()
            n = want["n_out"]
            print(f"state={state} key={key} {name} K={K}: pool {P}, kept {n}, walked {want['n_examined']}")
            assert (r.out.n_out, r.out.n_examined) == (n, want["n_examined"])
            keep = want["keep"]
            assert np.array_equal(r.index[:n], pool.index[keep])
            assert np.array_equal(r.key_value[:n], pool.key_value[keep])
            assert r.poses[:n].tobytes() == pool.poses[keep].tobytes()
            assert np.array_equal(r.corr[:n], pool.corr[keep]) and np.array_equal(r.n_corr[:n], pool.n_corr[keep])
            assert r.untouched(n)
            kept[(name, K)] = (n, r.out.n_examined)
    return P, kept


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("key", KEYS)
def test_suppression_equals_host_walk(state, key):
    eng, st, blobs, out = _stepped(70001, state)
    try:
        P, kept = _check_suppression(eng, state, key, blobs, SUPPRESS)
        assert P == 1024
        assert 1 < kept[("2mm", 1024)][0] < 1024                 # keeps many
        for K in (8, 1024):
            assert kept[("10m", K)] == (1, 1024)                 # keeps one and walks the whole pool
            assert kept[("rotation", K)] == (1, 1024)
    finally:
        eng.close()


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("key", KEYS)
def test_rotation_suppression_cuts_through_the_cloud(state, key):
    eng, st, blobs, out = _stepped(255, state)
    try:
        P, kept = _check_suppression(eng, state, key, blobs, SUPPRESS_SMALL)
        for name in SUPPRESS_SMALL:
            assert 1 < kept[(name, 1024)][0] <= P and kept[(name, 1024)][1] == P
        assert kept[("rotation 13 mrad", 1024)][0] < kept[("rotation 4 mrad", 1024)][0] < P  # some kept, some dropped
        assert kept[("both", 1024)][0] >= kept[("rotation 13 mrad", 1024)][0]                # and-ing separates more
    finally:
        eng.close()


# ---- 7. the chain: top_particles -> refine_poses
@pytest.mark.parametrize("state", STATES)
def test_chain_into_refine_poses(state):
    eng, st, blobs, out = _stepped(1000, state)
    try:
        top = eng.top_particles(key=pf.TOP_BY_WEIGHT, K=8, min_trans=0.002, blobs=blobs)
        assert top["n_out"] == 8
        got = eng.refine_poses(top["poses"], top["corr"], blobs=blobs)["rows"]
        for r in range(8):
            want = eng.refine_cloud(pf.ASSOC_PROPAGATED, blobs=blobs, first=int(top["index"][r]), count=1)["rows"]
            assert got[r].tobytes() == want[0].tobytes()
        # the same blobs as a frame of the staged bank
        eng.stage_blob_bank([blobs])
        bank = eng.top_particles(key=pf.TOP_BY_WEIGHT, K=8, min_trans=0.002, bank_frame=0)
        for k in ("index", "key_value", "poses", "corr", "n_corr"):
            assert bank[k].tobytes() == top[k].tobytes(), k
    finally:
        eng.close()


# ---- 8. no side effects
@pytest.mark.parametrize("fused", [2, 0])
def test_next_frame_is_unchanged_and_calls_repeat(fused):
    st = _stream(5, 50, 1000, 2)
    engs = [make_engine(1000, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX, fused=fused) for _ in range(2)]
    try:
        for e in engs:
            e.set_prior(st.prior(fast=True)[:1000])
            e.step(_frame(e, st.frames[0], 0))
        blobs = st.frames[0].blobs
        first = [Raw(engs[0], key, 64, min_trans=0.002, min_rot=0.5, blobs=blobs).rows() for key in KEYS]
        again = [Raw(engs[0], key, 64, min_trans=0.002, min_rot=0.5, blobs=blobs).rows() for key in KEYS]
        assert first == again
        outs = [e.step(_frame(e, st.frames[1], 1)) for e in engs]
        assert bytes(outs[0]) == bytes(outs[1])
        assert engs[0].get_particles(1).tobytes() == engs[1].get_particles(1).tobytes()
    finally:
        for e in engs:
            e.close()


# ---- 9. errors leave the outputs alone; the scratch outlives a larger particle set
def test_errors_leave_outputs_untouched():
    st = _stream(5, 50, 1000, 1)
    blobs = st.frames[0].blobs
    nan, inf = float("nan"), float("inf")

    def refused(r, code):
        assert r.rc == code, (r.rc, code)
        assert r.untouched() and (r.out_untouched())

    eng = pf.Engine(device=0, max_particles=1000, max_blobs=60, state_dtype=pf.STATE_F32)
    try:
        # before a model, a particle set or a step
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, blobs=blobs), pf.E_STATE)
        eng.set_model(st.markers, st.K)
        eng.set_prior(st.prior(fast=True)[:1000])
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8), pf.E_STATE)
        eng.step(_frame(eng, st.frames[0]))
        assert Raw(eng, pf.TOP_BY_WEIGHT, 8).rc == pf.OK
        refused(Raw(eng, pf.TOP_BY_COUNT, 8), pf.E_STATE)  # PFMPE_OPT_RECORD_COUNTS is off
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, ctx=False), pf.E_ARG)
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, null=("params",)), pf.E_ARG)
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, null=("out",)), pf.E_ARG)
        for key in (-1, 2):
            refused(Raw(eng, key, 8), pf.E_ARG)
        for K in (-1, pf.TOP_MAX + 1):
            refused(Raw(eng, pf.TOP_BY_WEIGHT, K), pf.E_ARG)
        for mt in (-0.001, inf, nan):
            refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, min_trans=mt), pf.E_ARG)
        for mr in (-0.001, math.pi + 1e-9, nan, inf):
            refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, min_rot=mr), pf.E_ARG)
        # blob descriptors pfmpe_get_pairs refuses: B < 0, no list with B > 0, a bank frame without a bank
        bad = _capi.AssocIn()
        bad.B, bad.bank_frame = -1, -1
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, ai=bad), pf.E_ARG)
        bad.B = 5
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, ai=bad), pf.E_ARG)
        bad.B, bad.bank_frame = 0, 3
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, ai=bad), pf.E_ARG)
        refused(Raw(eng, pf.TOP_BY_WEIGHT, 8, blobs=np.zeros((61, 2))), pf.E_CAP)
        eng.set_option(pf.OPT_RECORD_COUNTS, 1)
        eng.set_prior(st.prior(fast=True)[:1000])
        eng.step(_frame(eng, st.frames[0], blobs=np.zeros((0, 2))))  # a step that does not resample
        refused(Raw(eng, pf.TOP_BY_COUNT, 8), pf.E_STATE)
        assert Raw(eng, pf.TOP_BY_WEIGHT, pf.TOP_MAX, min_rot=math.pi).rc == pf.OK  # the edges of the ranges
    finally:
        eng.close()


def test_scratch_survives_a_larger_particle_set():
    st = _stream(5, 50, 70001, 1)
    eng = make_engine(70001, st.markers, st.K, pf.STATE_F32, pf.RNG_PHILOX)
    try:
        blobs = st.frames[0].blobs
        for N in (1000, 70001, 255):
            eng.set_prior(st.prior(fast=True)[:N])
            eng.step(_frame(eng, st.frames[0]))
            parts = eng.get_particles(0)
            corr, n_corr = eng.get_pairs(pf.ASSOC_PROPAGATED, blobs=blobs)
            for key in KEYS:
                k = _keys_of(eng, key)
                _check_ranking(eng, blobs, key, 1024, k, _ranking(k), parts, corr, n_corr)
    finally:
        eng.close()
