"""GPU tests of pfmpe_initialise_multi: the brute-force P3P (re)initialisation of S contexts as one batch.

The bar is the single call: out, the histogram and the seeded particle set of every stream equal what
pfmpe_initialise gives a twin engine with the same inputs, bit for bit (array_equal): the histogram counts are
order-free integer sums of per-item decisions taken by the same per-item code, and the host stages are the same
functions on the same inputs.  pfmpe_initialise is the batch of one, so the twins run the same kernels: these
comparisons show that the streams of a batch do not disturb each other (prefix tables, block plans, mixed buckets and
state types), not that the kernels are right.  That rests on the oracle: tests/test_gpu_init.py for the single call,
test_batch_matches_oracle here for a batch.
"""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

pytestmark = pytest.mark.gpu
K = syn.K_README
N = 200
# tests/test_gpu_init.py's CASES[:4]: (M, uniform outliers, near outliers, seed, noise px)
CASES = [(5, 3, 0, 0, 0.0), (5, 10, 2, 1, 0.3), (8, 3, 0, 6, 0.0), (6, 4, 1, 9, 0.3)]
F64, F32, F16 = pf.STATE_F64, pf.STATE_F32, pf.STATE_F16
OUT_KEYS = ("found", "flag_fail", "n_estimates", "n_candidates", "first_match", "hist_total")


def markers_of(M):
    if M <= 12:
        return syn.markers_for(M)
    extra = np.array([[0.11, -0.07, 0.05], [-0.13, 0.04, 0.09], [0.06, 0.12, -0.08], [-0.05, -0.11, 0.13]])
    return np.vstack([syn.markers_12(), extra])[:M]


def engine(M, state=F64, max_particles=256, max_blobs=pf.MAX_BLOBS):
    eng = pf.Engine(device=0, max_particles=max_particles, state_dtype=state, max_blobs=max_blobs)
    eng.set_model(markers_of(M), K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_REFERENCE
    eng.set_params(prm)
    return eng


def case_blobs(case):
    M, n_out, near, seed, noise = case
    return syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)[0]


def line_blobs(B=8):
    """Pairwise more than 1000 px apart: every 3-blob combination fails the spread filter (empty histogram)."""
    return np.array([[1001.0 * k, 240.0] for k in range(B)])


def some_prior(n=N, t=0.2):
    return np.tile(syn.to12(syn.truth_pose(t)), (n, 1))


def same_out(a, b):
    for k in OUT_KEYS:
        assert a[k] == b[k], (k, a[k], b[k])
    assert np.array_equal(a["pairs"], b["pairs"])
    assert np.array_equal(a["predicted_pose"], b["predicted_pose"])


def close_all(*lists):
    for lst in lists:
        for e in lst:
            e.close()


def six_streams(states):
    """CASES[:4], a stream with B = M - 1 (flag 10) and one with an empty histogram (flag 12); the last two hold a
    prior, so every stream has a particle set to compare afterwards.  Returns (engines, blob lists)."""
    Ms = [c[0] for c in CASES] + [5, 5]
    blobs = [case_blobs(c) for c in CASES] + [case_blobs(CASES[0])[:4], line_blobs()]
    engs = [engine(M, st) for M, st in zip(Ms, states)]
    for e in engs[4:]:
        e.set_prior(some_prior())
    return engs, blobs


@pytest.mark.parametrize("states", [[F64] * 6, [F64, F32, F16, F64, F32, F16]], ids=["f64", "mixed"])
def test_batch_equals_singles(states):
    batch, blobs = six_streams(states)
    twins, _ = six_streams(states)
    ref = [t.initialise(b, n_particles=N) for t, b in zip(twins, blobs)]
    got = pf.Engine.initialise_multi(batch, blobs, n_particles=N)
    assert [r[0]["flag_fail"] for r in ref] == [0, 0, 0, 0, 10, 12]
    for s in range(6):
        same_out(got[s][0], ref[s][0])
        assert np.array_equal(got[s][1], ref[s][1]), s
        assert np.array_equal(batch[s].get_particles(1), twins[s].get_particles(1)), s
    close_all(batch, twins)


def test_one_stream_equals_the_single_call():
    a, b = engine(5), engine(5)
    blobs = case_blobs(CASES[1])
    ref, h_ref = b.initialise(blobs, n_particles=N)
    (got, h), = pf.Engine.initialise_multi([a], [blobs], n_particles=N)
    assert ref["found"] == 1
    same_out(got, ref)
    assert np.array_equal(h, h_ref)
    assert np.array_equal(a.get_particles(1), b.get_particles(1))
    close_all([a, b])


def histogram_bars(h_gpu, M, blobs):
    """tests/test_gpu_init.py::test_histogram_matches_oracle's bars on one histogram; returns the oracle's."""
    h_gpu = h_gpu.astype(np.int64)
    h_ref, lo, hi, unbounded = orc.init_histogram_bounds(markers_of(M), K, blobs, tol=5.0)
    h_ref, lo, hi = h_ref.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)
    assert (h_gpu >= lo).all(), np.argwhere(h_gpu < lo)[:10]
    excess = np.maximum(h_gpu - hi, 0).sum()
    assert excess <= unbounded * (3 + M), (excess, unbounded)
    assert np.abs(h_gpu - h_ref).sum() <= max(4, 0.005 * h_ref.sum()), (np.abs(h_gpu - h_ref).sum(), h_ref.sum())
    return h_ref


def test_batch_matches_oracle():
    """The batch against the oracle, which runs none of its code: tests/test_gpu_init.py's bars, per stream
    (test_initialise_matches_oracle's on out and the seeded set, test_histogram_matches_oracle's on the histogram)."""
    cases = [CASES[0], CASES[2], CASES[3]]
    states = [("f64", F64), ("f32", F32), ("f16", F16)]
    inputs = [syn.init_blobs(c[0], c[1], c[3], noise_px=c[4], near=c[2]) for c in cases]
    blobs = [b for b, _ in inputs]
    engs = [engine(c[0], st) for c, (_, st) in zip(cases, states)]
    got = pf.Engine.initialise_multi(engs, blobs, n_particles=N)
    for s, (case, (name, _)) in enumerate(zip(cases, states)):
        M, near = case[0], case[2]
        out, h = got[s]
        assert h.sum() > 0
        histogram_bars(h, M, blobs[s])
        ref, _, parts = orc.initialise(markers_of(M), K, blobs[s], N, hist=h)
        for k in OUT_KEYS:
            assert out[k] == ref[k], (s, k, out[k], ref[k])
        assert np.array_equal(out["pairs"], ref["pairs"])
        assert out["found"] == 1
        np.testing.assert_allclose(out["predicted_pose"], ref["predicted_pose"], rtol=0, atol=1e-9)
        if near == 0:  # near-blob outliers can make the reference itself pick a wrong first match
            assert np.abs(syn.to44(out["predicted_pose"]) - inputs[s][1]).max() < 3e-2
        tol = {"f64": 1e-12, "f32": 4e-7, "f16": 1e-3}[name]
        np.testing.assert_allclose(engs[s].get_particles(1), parts, rtol=0, atol=tol)
    close_all(engs)


def test_histogram_only_below_M():
    """pfmpe_p3p_histogram computes the histogram for 3 <= B < M, where pfmpe_initialise stops at flag 10 and the
    public plan has no items: B = 3 (one combination, the smallest grid) and B = 4 (240 items, a partly filled
    block) at M = 5.  No combination can pass the >= 5-blob filter, so no floating-point decision is taken and the
    histogram is the oracle's entry for entry (all zero, by the oracle's word)."""
    M = 5
    b5 = case_blobs((M, 0, 0, 0, 0.0))
    eng = engine(M)
    for B in (3, 4):
        h = eng.p3p_histogram(b5[:B])
        assert h.shape == (B, M)
        h_ref = histogram_bars(h, M, b5[:B])
        assert np.array_equal(h.astype(np.int64), h_ref)
        assert pf.host_init_plan([M], [B], 256)[0][0]["items"] == 0  # the public plan follows pfmpe_initialise
    eng.set_prior(some_prior())
    before = eng.get_particles(1)
    out, _ = eng.initialise(b5[:4], n_particles=N)
    assert out["found"] == 0 and out["flag_fail"] == 10
    assert np.array_equal(eng.get_particles(1), before)
    eng.close()


def run_batch(engs, blobs, **kw):
    """(results or None, histograms, error or None): a candidate explosion leaves the histograms in the error."""
    try:
        res = pf.Engine.initialise_multi(engs, blobs, **kw)
        return res, [r[1] for r in res], None
    except pf.PFError as e:
        return None, e.hist, e


def test_block_cap_path():
    """One B = 50 stream beside two small ones: the plan of the batch is scaled down to the block cap."""
    blobs = [syn.init_blobs(5, 45, 2, noise_px=0.3)[0], case_blobs(CASES[0]), case_blobs(CASES[1])]
    batch, twins = [engine(5) for _ in blobs], [engine(5) for _ in blobs]
    num_cu = batch[0].info(pf.INFO_NUM_CU)
    assert num_cu >= 1
    plan, per_bucket = pf.host_init_plan([5, 5, 5], [len(b) for b in blobs], num_cu)
    wants = sum(-(-p["items"] // 256) for p in plan)
    assert wants > 8 * num_cu >= per_bucket[0] - 3  # the cap is hit: the test is not vacuous
    assert plan[0]["blocks"] < -(-plan[0]["items"] // 256)
    res, hists, err = run_batch(batch, blobs, n_particles=64)
    assert err is None or (err.code == pf.E_CAP and "stream 0" in str(err)), err
    for s in range(3):
        assert np.array_equal(hists[s], twins[s].p3p_histogram(blobs[s])), s
    if res is not None:
        for s in range(3):
            ref = twins[s].initialise(blobs[s], n_particles=64)[0]
            same_out(res[s][0], ref)
            if ref["found"]:
                assert np.array_equal(batch[s].get_particles(1), twins[s].get_particles(1))
        assert res[1][0]["found"] == 1 and res[2][0]["found"] == 1
    close_all(batch, twins)


def test_mixed_buckets():
    """M = 5, 8 and 16 in one batch: one histogram launch per unused-marker bucket.  The M = 16 set may be as
    self-similar as test_gpu_init.py's M = 12: then its candidate vectors pass the small max_candidates given here, the
    batch returns E_CAP for that stream after stage 1, and the histograms are what is compared (it does explode: the
    twin's single call decides which branch is checked)."""
    Ms = [5, 8, 16]
    T = syn.truth_pose(0.5)
    blobs = [case_blobs(CASES[0]), case_blobs(CASES[2]),
             syn.project(K, T, markers_of(16)).astype(np.float32).astype(np.float64)]
    batch, twins = [engine(M) for M in Ms], [engine(M) for M in Ms]
    for e in batch:
        e.set_prior(some_prior())
    before = [e.get_particles(1) for e in batch]
    caps = [1 << 20, 1 << 20, 1000]
    explodes = False
    try:
        ref2 = twins[2].initialise(blobs[2], n_particles=N, max_candidates=caps[2])
    except pf.PFError as e:
        assert e.code == pf.E_CAP
        explodes = True
    res, hists, err = run_batch(batch, blobs, n_particles=N, max_candidates=caps)
    print("M = 16 candidate stage explodes:", explodes)
    for s in range(3):
        assert hists[s].sum() > 0
        assert np.array_equal(hists[s], twins[s].p3p_histogram(blobs[s])), s
    if explodes:
        assert err is not None and err.code == pf.E_CAP
        assert "initialise_multi: stream 2: " in str(err) and "max_candidates" in str(err)
        for s in range(3):  # no context was seeded
            assert np.array_equal(batch[s].get_particles(1), before[s])
    else:
        assert err is None
        for t in twins[:2]:
            t.set_prior(some_prior())
        twins[2].set_prior(some_prior())
        ref = [twins[s].initialise(blobs[s], n_particles=N, max_candidates=caps[s]) for s in range(2)] + [ref2]
        for s in range(3):
            same_out(res[s][0], ref[s][0])
    close_all(batch, twins)


def test_prior_handling():
    """Slot 0 per stream: a found member keeps its resident slot 0, or gets the identity without a prior; a member
    that is not found keeps its whole set."""
    blobs = [case_blobs(CASES[0]), case_blobs(CASES[1]), case_blobs(CASES[0])[:4]]
    engs = [engine(5) for _ in blobs]
    prior = syn.initial_prior(syn.truth_pose(0.2), N, seed=3)
    engs[0].set_prior(prior)
    engs[2].set_prior(prior)
    kept = engs[2].get_particles(1)
    res = pf.Engine.initialise_multi(engs, blobs, n_particles=N)
    assert [r[0]["found"] for r in res] == [1, 1, 0] and res[2][0]["flag_fail"] == 10
    assert res[0][0]["n_estimates"] < N  # K < N: the slot-0 rule applies
    assert np.array_equal(engs[0].get_particles(1)[0], prior[0])
    assert np.array_equal(engs[1].get_particles(1)[0], np.eye(4)[:3].reshape(12))
    assert np.array_equal(engs[2].get_particles(1), kept)
    assert engs[2].info(pf.INFO_N) == N
    close_all(engs)


def test_then_track():
    """pfmpe_step_multi on batch-initialised contexts equals pfmpe_step_multi on contexts initialised one by one."""
    cases = [CASES[0], CASES[1]]
    blobs = [case_blobs(c) for c in cases]
    batch, twins = [engine(5) for _ in cases], [engine(5) for _ in cases]
    got = pf.Engine.initialise_multi(batch, blobs, n_particles=N)
    ref = [t.initialise(b, n_particles=N) for t, b in zip(twins, blobs)]
    nb = syn.project(K, syn.truth_pose(0.5), syn.markers_for(5)) + 0.3
    eye = np.eye(4)[:3].reshape(12)

    def frames(engs, outs):
        return [e.make_frame(o[0]["predicted_pose"], o[0]["predicted_pose"], eye, blobs=nb, it_since_init=1, dt=0.02,
                             seed=77 + s) for s, (e, o) in enumerate(zip(engs, outs))]

    o_b = pf.Engine.step_multi(batch, frames(batch, got))
    o_t = pf.Engine.step_multi(twins, frames(twins, ref))
    for s in range(2):
        a, b = o_b[s].as_dict(), o_t[s].as_dict()
        for k in ("iters", "kept_iter", "accepted", "resampled", "most_likely_idx", "winner_idx", "n_corr", "flag_fail"):
            assert a[k] == b[k], (s, k)
        assert np.array_equal(a["pairs"], b["pairs"])
        assert np.array_equal(batch[s].get_weights(), twins[s].get_weights())
    close_all(batch, twins)


def raw_call(engs, S, Bs, blob_arrays, n_particles, null_blobs=(), null_out=False, null_in=False, ctx_override=None):
    """pfmpe_initialise_multi through ctypes with a sentinel-filled out array; returns (code, out bytes)."""
    lib = pf.load()
    ctx_vals = [e.ctx.value if e is not None else None for e in engs] if ctx_override is None else ctx_override
    ctxs = (C.c_void_p * len(ctx_vals))(*ctx_vals)
    ins, ips, outs = (pf.InitIn * S)(), (pf.InitParams * S)(), (pf.InitOut * S)()
    C.memset(outs, 0x5A, C.sizeof(outs))
    for s in range(S):
        a = blob_arrays[s % len(blob_arrays)]
        ins[s].blobs = C.POINTER(C.c_double)() if s in null_blobs else a.ctypes.data_as(C.POINTER(C.c_double))
        ins[s].B = Bs[s % len(Bs)]
        lib.pfmpe_default_init_params(C.byref(ips[s]))
        ips[s].n_particles = n_particles[s % len(n_particles)]
    rc = lib.pfmpe_initialise_multi(ctxs, S, None if null_in else ins, ips, None if null_out else outs, None)
    return rc, bytes(outs)


def test_errors_leave_everything_untouched():
    blobs = np.ascontiguousarray(case_blobs(CASES[0]))
    B = len(blobs)
    a, b = engine(5), engine(5)
    small = engine(5, max_blobs=6)
    two = pf.Engine(device=0, max_particles=256, state_dtype=F64)
    two.set_model(syn.markers_for(5)[:2], K)
    bare = pf.Engine(device=0, max_particles=256, state_dtype=F64)
    for e in (a, b, small, two):
        e.set_prior(some_prior(64))
    before = {e: e.get_particles(1) for e in (a, b, small, two)}
    sentinel = bytes([0x5A]) * C.sizeof(pf.InitOut)
    # (engines, S, B per stream, n_particles per stream, extra, code, stream named in the text or None)
    rows = [
        ([a, b], 2, [B, -1], [64], {}, pf.E_ARG, 1),
        ([a, b], 2, [B, B], [64], {"null_blobs": (1,)}, pf.E_ARG, 1),
        ([a, None], 2, [B], [64], {}, pf.E_ARG, 1),
        ([a, b, a], 3, [B], [64], {}, pf.E_ARG, 2),
        ([a, two], 2, [B], [64], {}, pf.E_ARG, 1),
        ([a, bare], 2, [B], [64], {}, pf.E_STATE, 1),
        ([a, small], 2, [B], [64], {}, pf.E_CAP, 1),
        ([b, a], 2, [B], [64, 100000], {}, pf.E_CAP, 1),
        ([a] * 65, 65, [B], [64], {}, pf.E_CAP, None),
        ([a, b], 2, [B], [64], {"null_out": True}, pf.E_ARG, None),
        ([a, b], 2, [B], [64], {"null_in": True}, pf.E_ARG, None),
    ]
    for engs, S, Bs, nps, extra, code, stream in rows:
        rc, raw = raw_call(engs, S, Bs, [blobs], nps, **extra)
        assert rc == code, (rc, code, stream)
        assert raw == sentinel * S
        text = engs[0].last_error()
        assert text.startswith("initialise_multi: "), text
        if stream is not None:
            assert f"stream {stream}: " in text, text
    # S < 1, ctxs[0] = NULL: PFMPE_E_ARG with no text
    assert raw_call([a], 1, [B], [blobs], [64], ctx_override=[None])[0] == pf.E_ARG
    lib = pf.load()
    assert lib.pfmpe_initialise_multi((C.c_void_p * 1)(a.ctx.value), 0, None, None, None, None) == pf.E_ARG
    assert lib.pfmpe_initialise_multi(None, 1, None, None, None, None) == pf.E_ARG
    for e, p in before.items():
        assert np.array_equal(e.get_particles(1), p)
        assert e.info(pf.INFO_N) == 64
    close_all([a, b, small, two, bare])


def test_timing_is_the_leaders():
    blobs = [case_blobs(c) for c in CASES[:3]]
    engs = [engine(c[0]) for c in CASES[:3]]
    engs[0].set_option(pf.OPT_TIMING, 1)
    for e in engs:
        e.reset_kernel_stats()
    for n in (1, 2):
        pf.Engine.initialise_multi(engs, blobs, n_particles=N)
        st = engs[0].kernel_stats()
        assert st["k_p3p_hist"][0] == n and st["k_p3p_check"][0] == n, st  # one bracket of each per batch
        assert st["k_p3p_hist"][1] > 0
    for e in engs[1:]:
        assert all(v[0] == 0 for v in e.kernel_stats().values())
    close_all(engs)


def test_ordering_with_a_members_own_stream():
    """A member steps on its own stream, is re-initialised in a batch led by another context, and steps again: the
    three results equal the same sequence done with single calls."""
    blobs = [case_blobs(CASES[1]), case_blobs(CASES[0])]
    nb = syn.project(K, syn.truth_pose(0.5), syn.markers_for(5)) + 0.3
    eye = np.eye(4)[:3].reshape(12)
    prior = syn.initial_prior(syn.truth_pose(0.5), N, seed=5)
    cur = syn.to12(syn.truth_pose(0.5))

    def sequence(batched):
        lead, mem = engine(5), engine(5)
        mem.set_prior(prior)
        o1 = mem.step(mem.make_frame(cur, cur, eye, blobs=nb, dt=0.02, seed=5)).as_dict()
        if batched:
            init = pf.Engine.initialise_multi([lead, mem], blobs, n_particles=N)[1]
        else:
            lead.initialise(blobs[0], n_particles=N)
            init = mem.initialise(blobs[1], n_particles=N)
        pp = init[0]["predicted_pose"]
        o2 = mem.step(mem.make_frame(pp, pp, eye, blobs=nb, it_since_init=1, dt=0.02, seed=6)).as_dict()
        res = (o1, init, o2, mem.get_weights(), mem.get_particles(1))
        close_all([lead, mem])
        return res

    a, b = sequence(True), sequence(False)
    for oa, ob in ((a[0], b[0]), (a[2], b[2])):
        for k, v in oa.items():
            assert np.array_equal(v, ob[k]), k
    same_out(a[1][0], b[1][0])
    assert np.array_equal(a[1][1], b[1][1])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
