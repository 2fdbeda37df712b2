"""pfmpe_resample_prior on the device: the rows of the new prior against the engine's own read-back indexed by
pfmpe_host_resample_source (the same integer rule on both sides, the members by pfmpe_host_cloud_assign: the function
the device runs), bit for bit for every state type; what the call leaves of dst and src; and its errors.  Everything is
a copy of stored elements or an integer, so every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi
from test_gpu_parity import make_engine
from test_gpu_top import _stepped, _stream, _frame

import cloud_modes_ref as ref

pytestmark = pytest.mark.gpu

STATES = [pf.STATE_F64, pf.STATE_F32, pf.STATE_F16]
NONE = pf.MODE_NONE
TS, RS = ref.TRANS_SCALE, ref.ROT_SCALE
DP = C.POINTER(C.c_double)
SENT = (-11, -12, -13)


def _prior_engine(N, state, cap=None, fused=2, rows=None):
    """An engine of max_particles `cap` whose prior is the first N particles of the three-mode cloud."""
    st = _stream(5, 50, 1000, 1)
    eng = make_engine(max(N, cap or N), st.markers, st.K, state, pf.RNG_PHILOX, fused=fused)
    eng.set_prior(ref.cloud(300_001, 1)[:N] if rows is None else rows)
    return eng


def _bare_engine(cap, state):
    """A context with no model and no prior."""
    return pf.Engine(device=0, max_particles=cap, state_dtype=state)


class Raw:
    """One C call with a sentinel in every field of `out`; keeps the Python engine's N in step on success."""

    def __init__(self, dst, src, n_new, seeds=None, mode=0, prm=(TS, RS, 0.0), K=None, null=(), ctx=True):
        self.out = _capi.ResampleOut(*SENT)
        p = _capi.ResampleParams()
        p.n_new = int(n_new)
        self._seeds = None
        if seeds is not None:
            self._seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.float64).reshape(-1, 12))
            p.K, p.seeds = self._seeds.shape[0], self._seeds.ctypes.data_as(DP)
        if K is not None:
            p.K = K
        if "seeds" in null:
            p.seeds = None
        p.mode = int(mode)
        p.modes = _capi.ModesParams(*prm)
        self.rc = dst.lib.pfmpe_resample_prior(
            dst.ctx if ctx else None, None if "src" in null else src.ctx, None if "params" in null else C.byref(p),
            None if "out" in null else C.byref(self.out))
        if self.rc == pf.OK and self.out.n_new > 0:
            dst.N = int(self.out.n_new)
            dst._last_out = None

    def result(self):
        return (self.out.n_src, self.out.n_members, self.out.n_new)

    def untouched(self):
        return self.result() == SENT


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_all(dst, src, n_new):
    """No filter: dst's rows after == src's rows before [source], out and PFMPE_INFO_N."""
    before = src.get_particles(1)
    N = len(before)
    source, m = pf.host_resample_source(None, 0, n_new, N=N)
    r = Raw(dst, src, n_new)
    assert r.rc == pf.OK, dst.last_error()
    assert r.result() == (N, N, n_new) and m == N
    assert dst.info(pf.INFO_N) == n_new
    assert _same(dst.get_particles(1), before[source])
    if dst is not src:
        assert src.info(pf.INFO_N) == N and _same(src.get_particles(1), before)


def _check_mode(dst, src, seeds, mode, n_news, prm=(TS, RS, 0.0), before=None):
    """With a filter: m and source from the engine's own read-back through pfmpe_host_cloud_assign.  n_news: a function
    of (m, N).  dst is not src (src is read once and stays).  Returns m."""
    assert dst is not src
    before = src.get_particles(1) if before is None else before
    N = len(before)
    mode_of, counts = pf.host_cloud_assign(before, seeds, trans_scale=prm[0], rot_scale=prm[1], max_dist=prm[2])
    m = int(counts[len(seeds) if mode == NONE else mode])
    assert m > 0
    for n_new in n_news(m, N):
        if n_new < 1:
            continue
        source, got_m = pf.host_resample_source(mode_of, mode, n_new)
        assert got_m == m
        r = Raw(dst, src, n_new, seeds, mode, prm)
        assert r.rc == pf.OK, dst.last_error()
        assert r.result() == (N, m, n_new), (mode, n_new)
        assert dst.info(pf.INFO_N) == n_new
        assert _same(dst.get_particles(1), before[source]), (mode, n_new)
    return m


AROUND = lambda m, N: (m - 1, m, m + 1, 2 * N)  # noqa: E731


# ---- 1. rows, no filter
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N,n_new", [(1, 1), (1, 257), (257, 1), (255, 256), (256, 255), (257, 4097), (4097, 257),
                                     (4097, 4097)])
def test_rows_without_a_filter(N, n_new, state):
    """In place: one lane, a block less one, a block, a block plus one, 17 blocks, shrinking, growing and the identity."""
    eng = _prior_engine(N, state, cap=max(N, n_new))
    try:
        _check_all(eng, eng, n_new)
        _check_all(eng, eng, N)  # and back to N particles from the set just made
    finally:
        eng.close()


# ---- 2. rows, with a filter
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("N", [255, 256, 257, 4097])
def test_rows_with_a_filter(N, state):
    """Modes 0, 1, 2 ungated and the particles no seed takes under the gate 12.0, each to m - 1, m, m + 1 and 2 N new
    particles in another context; the last one in place as well."""
    seeds = ref.seeds(3)
    src = _prior_engine(N, state, cap=2 * N)
    dst = _bare_engine(2 * N, state)
    try:
        before = src.get_particles(1)
        ms = [_check_mode(dst, src, seeds, mode, AROUND, before=before) for mode in (0, 1, 2)]
        assert sum(ms) == N and min(ms) > N // 6
        m = _check_mode(dst, src, seeds, NONE, AROUND, prm=(TS, RS, 12.0), before=before)
        assert N // 4 < m < N
        assert _same(src.get_particles(1), before) and src.info(pf.INFO_N) == N
        # in place: the leftover of the gate, doubled
        mode_of, _ = pf.host_cloud_assign(before, seeds, trans_scale=TS, rot_scale=RS, max_dist=12.0)
        source, _ = pf.host_resample_source(mode_of, NONE, 2 * m)
        r = Raw(src, src, 2 * m, seeds, NONE, (TS, RS, 12.0))
        assert r.rc == pf.OK and r.result() == (N, m, 2 * m)
        assert _same(src.get_particles(1), before[source])
    finally:
        src.close()
        dst.close()


# ---- 3. no members
@pytest.mark.parametrize("state", STATES)
def test_no_members_changes_nothing(state):
    """N = 1: the one particle is mode 1, so mode 0 has no member: PFMPE_OK, out = (1, 0, 0), and dst (stepped: prior, N,
    kept propagated set) is as it was; in place the same."""
    seeds = ref.seeds(3)
    src = _prior_engine(1, state)
    dst, st, blobs, out = _stepped(257, state)
    try:
        _, counts = pf.host_cloud_assign(src.get_particles(1), seeds, trans_scale=TS, rot_scale=RS)
        assert list(counts) == [0, 1, 0, 0]
        prior, kept, w = dst.get_particles(1), dst.get_particles(0), dst.get_weights()
        for d in (dst, src):
            own = d.get_particles(1)
            r = Raw(d, src, 5 if d is dst else 1, seeds, 0)
            assert r.rc == pf.OK and r.result() == (1, 0, 0)
            assert d.info(pf.INFO_N) == len(own) and _same(d.get_particles(1), own)
        assert _same(dst.get_particles(1), prior) and _same(dst.get_particles(0), kept) and _same(dst.get_weights(), w)
        # and the member does move
        r = Raw(dst, src, 5, seeds, 1)
        assert r.rc == pf.OK and r.result() == (1, 1, 5)
        assert _same(dst.get_particles(1), np.repeat(src.get_particles(1), 5, axis=0))
    finally:
        src.close()
        dst.close()


def _own_seeds(rows):
    """Two seeds of a posterior: its first particle and the one farthest from it; the scale is half their distance."""
    d = np.linalg.norm(rows[:, ref.T_IDX] - rows[0, ref.T_IDX], axis=1)
    far = int(np.argmax(d))
    assert d[far] > 0
    return np.stack([rows[0], rows[far]]), (d[far] / 2, 0.2, 0.0)


# ---- 4. a deferred prior
@pytest.mark.parametrize("state", STATES)
def test_deferred_prior_is_read_through_its_owners(state):
    N = 4097
    src, st, blobs, out = _stepped(N, state, fused=0)
    dst = _bare_engine(2 * N, state)
    try:
        assert out.resampled and src.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS
        before = src.get_particles(1)
        for n_new in (257, N, 2 * N):
            _check_all(dst, src, n_new)
        seeds, prm = _own_seeds(before)
        ms = [_check_mode(dst, src, seeds, mode, AROUND, prm=prm, before=before) for mode in (0, 1)]
        assert sum(ms) == N
        assert _same(src.get_particles(1), before) and _same(src.get_particles(0), src.get_particles(0))
    finally:
        src.close()
        dst.close()


def _next_steps(eng, st, frames=(1, 2)):
    """The records and priors of the next steps, as bytes."""
    res = []
    for f in frames:
        out = eng.step(_frame(eng, st.frames[f], f))
        res.append((bytes(out), eng.get_particles(1).tobytes()))
    return res


def _stepped_cap(N, cap, state, fused):
    """_stepped with room for `cap` particles and a stream of three frames."""
    st = _stream(5, 50, max(N, 1000), 3)
    eng = make_engine(cap, st.markers, st.K, state, pf.RNG_PHILOX, fused=fused)
    eng.set_prior(st.prior(fast=True)[:N])
    out = eng.step(_frame(eng, st.frames[0]))
    return eng, st, out


# ---- 5. the identity changes nothing downstream
@pytest.mark.parametrize("fused", [0, 2])
@pytest.mark.parametrize("state", STATES)
def test_identity_changes_nothing_downstream(state, fused):
    """n_new = N of every particle copies the prior into the other state buffer (for fp16 with its anchor, the deltas
    raw; with PFMPE_OPT_FUSED = 0 out of a deferred prior): the next two steps return the twin's bytes."""
    N = 4097
    a, st, _ = _stepped_cap(N, N, state, fused)
    b, _, _ = _stepped_cap(N, N, state, fused)
    try:
        assert a.resample_prior(N) == {"n_src": N, "n_members": N, "n_new": N}
        with pytest.raises(pf.PFError) as e:  # the kept set of the earlier step is gone
            a.get_particles(0)
        assert e.value.code == pf.E_STATE
        assert _same(a.get_particles(1), b.get_particles(1))
        assert _next_steps(a, st) == _next_steps(b, st)
    finally:
        a.close()
        b.close()


# ---- 6. a changed N behaves like set_prior
@pytest.mark.parametrize("n_new", [1000, 8000])
@pytest.mark.parametrize("state", [pf.STATE_F64, pf.STATE_F32])
def test_changed_count_behaves_like_set_prior(state, n_new):
    """The twin, of the same max_particles and history, gets the same rows through pfmpe_set_prior: the next two steps
    have byte-equal records and priors.  fp64 and fp32 only: for fp16 state pfmpe_set_prior re-anchors the set at its
    first particle, while the resampled set keeps the anchor it had, so the stored deltas differ (not tested)."""
    N, cap = 4097, 8000
    a, st, _ = _stepped_cap(N, cap, state, 2)
    b, _, _ = _stepped_cap(N, cap, state, 2)
    try:
        rows = a.get_particles(1)
        source, m = pf.host_resample_source(None, 0, n_new, N=N)
        assert a.resample_prior(n_new) == {"n_src": N, "n_members": N, "n_new": n_new}
        b.set_prior(rows[source])
        assert a.info(pf.INFO_N) == b.info(pf.INFO_N) == n_new
        assert _same(a.get_particles(1), b.get_particles(1))
        assert _next_steps(a, st) == _next_steps(b, st)
    finally:
        a.close()
        b.close()


# ---- 7. fork
@pytest.mark.parametrize("state", STATES)
def test_fork_leaves_src_untouched(state):
    """dst: another max_particles, no model, no prior.  src (stepped) keeps its prior bytes and its kept set: its WEIGHTED
    statistics return the bytes they returned before.  Then the roles swap: the fork, whose latest work went to its
    own stream, is the source of the first context's new prior."""
    N = 4097
    src, st, blobs, out = _stepped(N, state)
    dst = _bare_engine(3 * N + 5, state)
    try:
        before = src.get_particles(1)
        ref_pose = np.array(out.winner_pose if out.resampled else out.most_likely_pose)
        stats = {k: np.asarray(v).tobytes() for k, v in src.cloud_stats(pf.CLOUD_WEIGHTED, ref_pose).items()}
        seeds, prm = _own_seeds(before)
        _check_mode(dst, src, seeds, 1, AROUND, prm=prm, before=before)
        _check_mode(dst, src, seeds, 0, lambda m, N: (3 * N + 5,), prm=prm, before=before)
        assert _same(src.get_particles(1), before) and src.info(pf.INFO_N) == N
        again = {k: np.asarray(v).tobytes() for k, v in src.cloud_stats(pf.CLOUD_WEIGHTED, ref_pose).items()}
        assert again == stats
        # the roles swapped: dst's 3 N + 5 particles (copies of mode 0) back into src, filtered and not
        forked = dst.get_particles(1)
        dst.cloud_stats(pf.CLOUD_POSTERIOR, ref_pose)  # the fork's latest work: on its own stream
        _check_mode(src, dst, seeds, 0, lambda m, N: (N // 4,), prm=prm, before=forked)
        _check_all(src, dst, N)
        assert _same(dst.get_particles(1), forked)
        src.step(_frame(src, st.frames[0]))  # and the first context still steps
    finally:
        src.close()
        dst.close()


# ---- 8. seams
def _tiled_cloud(N):
    base = ref.cloud(300_001, 1)
    return np.tile(base, (-(-N // len(base)), 1))[:N]


def test_seam_many_blocks_f16():
    """N = 1024 * 256 + 37 fp16 particles (four super-blocks and a part) to 131072, unfiltered and keeping mode 1 of
    three."""
    N, n_new = 1024 * 256 + 37, 131072
    src = _prior_engine(N, pf.STATE_F16)
    dst = _bare_engine(n_new, pf.STATE_F16)
    try:
        before = src.get_particles(1)
        _check_all(dst, src, n_new)
        _, counts = pf.host_cloud_assign(before, ref.seeds(3), trans_scale=TS, rot_scale=RS)
        print("members", list(counts))  # 87412 / 87394 / 87375 for the fp64 rows
        assert min(counts[:3]) > 80_000
        _check_mode(dst, src, ref.seeds(3), 1, lambda m, N: (n_new,), before=before)
    finally:
        src.close()
        dst.close()


def test_seam_super_block():
    """N = 65536 + 257: the second super-block of the block prefix (256 blocks of 256 particles form one) holds one
    full block and one particle; modes 0 and 2 shrink, mode 1 grows."""
    N = 65536 + 257
    src = _prior_engine(N, pf.STATE_F32)
    dst = _bare_engine(N, pf.STATE_F32)
    try:
        before = src.get_particles(1)
        for mode, f in ((0, lambda m, N: (m - 1, 1000)), (1, lambda m, N: (N,)), (2, lambda m, N: (m,))):
            _check_mode(dst, src, ref.seeds(3), mode, f, before=before)
    finally:
        src.close()
        dst.close()


def test_seam_grid_cap():
    """Both gathers run at most 2048 blocks of 256 lanes and stride beyond: 2048 * 256 + 37 new slots from 4097
    particles (unfiltered, the slots' grid), and 2048 * 256 + 300 source particles filtered (the members' grid)."""
    cap = 2048 * 256
    small = _prior_engine(4097, pf.STATE_F16)
    big = _bare_engine(cap + 300, pf.STATE_F16)
    try:
        _check_all(big, small, cap + 37)
        big.set_prior(_tiled_cloud(cap + 300))
        before = big.get_particles(1)
        _check_mode(small, big, ref.seeds(3), 2, lambda m, N: (4097, 1), before=before)
    finally:
        small.close()
        big.close()


def test_seam_top_scan_width():
    """The scan over the super-blocks' sums takes 64 of them per trip: N = 64 * 65536 + 257 has a 65th."""
    N = 64 * 65536 + 257
    src = _prior_engine(N, pf.STATE_F16, rows=_tiled_cloud(N))
    dst = _bare_engine(5000, pf.STATE_F16)
    try:
        before = src.get_particles(1)
        m = _check_mode(dst, src, ref.seeds(3), 2, lambda m, N: (4999,), before=before)
        assert m > N // 4
        _check_all(dst, src, 5000)
    finally:
        src.close()
        dst.close()


# ---- 9. errors
def test_errors_and_their_texts():
    N = 300
    seeds = ref.seeds(3)
    nan_seed = seeds.copy()
    nan_seed[1, 5] = np.nan
    nan, inf = float("nan"), float("inf")
    SCALE = "resample_prior: a scale or max_dist is negative or not finite"
    src = _prior_engine(N, pf.STATE_F32)
    dst = _prior_engine(N, pf.STATE_F32, rows=ref.cloud(300_001, 1)[1000:1000 + N])
    empty = _bare_engine(N, pf.STATE_F32)
    other = _prior_engine(N, pf.STATE_F16)
    try:
        prior = dst.get_particles(1)

        def fails(code, text, d=dst, s=src, n_new=100, **kw):
            r = Raw(d, s, n_new, **kw)
            assert (r.rc, d.last_error()) == (code, text)
            assert text.startswith("resample_prior: ") and r.untouched()

        assert Raw(dst, src, 100, ctx=False).rc == pf.E_ARG  # no dst: no text
        for null in ("src", "params", "out"):
            fails(pf.E_ARG, "resample_prior: bad arguments", null=(null,))
        for n in (0, -1):
            fails(pf.E_ARG, "resample_prior: n_new < 1", n_new=n)
        fails(pf.E_ARG, "resample_prior: device and state type of src must match dst", s=other)
        fails(pf.E_ARG, "resample_prior: device and state type of src must match dst", d=other)
        for K in (-1, pf.MODES_MAX + 1):
            fails(pf.E_ARG, "resample_prior: K outside 0..PFMPE_MODES_MAX", seeds=ref.seeds(16), K=K)
        fails(pf.E_ARG, "resample_prior: null seeds", seeds=seeds, null=("seeds",))
        fails(pf.E_ARG, "resample_prior: non-finite seed", seeds=nan_seed)
        for prm in ((-0.01, 0.05, 0.0), (nan, 0.05, 0.0), (0.01, inf, 0.0), (0.01, 0.05, -1.0), (0.01, 0.05, nan)):
            fails(pf.E_ARG, SCALE, seeds=seeds, prm=prm)
        fails(pf.E_ARG, "resample_prior: both scales are 0", seeds=seeds, prm=(0.0, 0.0, 1.0))
        for mode in (-1, 3, 254, 256):
            fails(pf.E_ARG, "resample_prior: mode is neither 0..K-1 nor PFMPE_MODE_NONE", seeds=seeds, mode=mode)
        fails(pf.E_CAP, "resample_prior: n_new exceeds max_particles", n_new=N + 1)
        fails(pf.E_STATE, "resample_prior: no particle set", s=empty)
        fails(pf.E_STATE, "resample_prior: no particle set", d=empty, s=empty)
        # the argument checks come before the state check
        fails(pf.E_ARG, "resample_prior: n_new < 1", s=empty, n_new=0)
        assert _same(dst.get_particles(1), prior) and dst.info(pf.INFO_N) == N
        assert empty.info(pf.INFO_N) == 0
        with pytest.raises(pf.PFError) as e:
            dst.resample_prior(N + 1, src=src)
        assert e.value.code == pf.E_CAP
        # and what is allowed: with K = 0 seeds, mode and scales are ignored; NONE without a gate has no member
        r = Raw(dst, src, 100, prm=(nan, -1.0, inf), mode=99)
        assert r.rc == pf.OK and r.result() == (N, N, 100)
        r = Raw(dst, src, 50, seeds, NONE)
        assert r.rc == pf.OK and r.result() == (N, 0, 0) and dst.info(pf.INFO_N) == 100
        got = empty.resample_prior(N, src=src, seeds=seeds, mode=1, max_dist=12.0)
        assert got["n_src"] == N and 0 < got["n_members"] < N and got["n_new"] == N and empty.N == N
    finally:
        for e in (src, dst, empty, other):
            e.close()
