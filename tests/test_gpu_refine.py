"""pfmpe_refine_poses / pfmpe_refine_cloud on the device: rows against pfmpe_host_optimise_pose (LIST) and against the
oracle's optimisePose on the engine's own particles and pairs (CLOUD) under the rules of refine_ref.py; the summary
against the rows; ranges, repeated calls, bank frames, frame state, errors; and the closed loop with the winner refined
by the engine."""
import ctypes

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

import refine_ref as rr

pytestmark = pytest.mark.gpu

STATES = {"f64": pf.STATE_F64, "f32": pf.STATE_F32, "f16": pf.STATE_F16}


def make_engine(markers, K, N, state=pf.STATE_F64, prior=None, rng=pf.RNG_PHILOX):
    eng = pf.Engine(device=0, max_particles=max(N, 1), state_dtype=state)
    eng.set_model(markers, K)
    prm = pf.default_params()
    prm.rng_mode = rng
    eng.set_params(prm)
    if prior is not None:
        eng.set_prior(prior)
    return eng


def host_ref(markers, K, blobs, poses, pairs, params=None):
    """pfmpe_host_optimise_pose over the hypotheses, as a reference dict for rr.compare."""
    n = len(poses)
    rows = np.zeros(n, dtype=pf.REFINE_ROW_DTYPE)
    cov = np.zeros((n, 6, 6))
    for i in range(n):
        rows[i], cov[i] = pf.host_optimise_pose(markers, K, blobs, pairs[i], poses[i], params)
    ref = {"pose": rows["pose"], "cov": cov, "iters": rows["iters"], "n_pairs": rows["n_pairs"],
           "rms_before": rows["rms_before"], "rms_after": rows["rms_after"], "status": rows["status"]}
    return rows, ref


def best_of(rows):
    """numpy argbest: most pairs, then the smallest rms_after, then the lowest index; -1 if no row takes part."""
    ok = np.flatnonzero((rows["n_pairs"] > 0) & np.isfinite(rows["rms_after"]))
    if len(ok) == 0:
        return -1
    order = np.lexsort((ok, rows["rms_after"][ok], -rows["n_pairs"][ok].astype(np.int64)))
    return int(ok[order[0]])


def check_summary(res, rows, cov):
    """The summary of a call against its full-range rows."""
    assert res["n"] == len(rows)
    assert res["n_with_pairs"] == int(np.count_nonzero(rows["n_pairs"] > 0))
    assert res["n_converged"] == int(np.count_nonzero(rows["status"] == pf.REFINE_CONVERGED))
    assert res["n_cap_kept"] == int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_KEPT))
    assert res["n_cap_reverted"] == int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_REVERTED))
    assert res["iters_total"] == int(rows["iters"].astype(np.int64).sum())
    assert res["iters_max"] == (int(rows["iters"].max()) if len(rows) else 0)
    b = best_of(rows)
    assert res["best"] == b
    if b >= 0:
        assert res["best_row"].tobytes() == rows[b].tobytes()
        assert res["best_cov"].tobytes() == cov[b].tobytes()
    else:
        assert not np.frombuffer(res["best_row"].tobytes(), dtype=np.uint8).any() and not res["best_cov"].any()


def summary_bytes(res):
    return b"".join([np.array([res[k] for k in ("n", "n_with_pairs", "n_converged", "n_cap_kept", "n_cap_reverted",
                                                "iters_total", "iters_max", "best")], dtype=np.int64).tobytes(),
                     res["best_row"].tobytes(), res["best_cov"].tobytes()])


# ------------------------------------------------------------------------------------------------------- LIST
@pytest.mark.parametrize("name,k", [("A", 1), ("B", 65), ("C", 700), ("A", 700)])
def test_list_against_host(name, k):
    markers, K, blobs, poses, pairs, oref = rr.cloud(name)
    if k == 1:  # one hypothesis with every LED paired
        sel = np.flatnonzero(oref["n_pairs"] == len(markers))[:1]
    else:
        sel = np.arange(k)
    poses, pairs = poses[sel], pairs[sel]
    hrows, href = host_ref(markers, K, blobs, poses, pairs)
    eng = make_engine(markers, K, 1000)
    try:
        res = eng.refine_poses(poses, pairs, blobs=blobs, want_cov=True)
        again = eng.refine_poses(poses, pairs, blobs=blobs, want_cov=True)
        norows = eng.refine_poses(poses, pairs, blobs=blobs)
    finally:
        eng.close()
    rows, cov = res["rows"], res["cov"]
    print(f"{name}: oracle under +-1 ulp: cov spread {oref['cov_spread']:.3e}, pose spread {oref['pose_spread_determined']:.3e} m "
          f"(>= 3 pairs) / {oref['pose_spread_undetermined']:.3e} m (1-2 pairs)")
    rr.compare(f"list {name} K={k}", rows, cov, href, hrows["status"] == pf.REFINE_CONVERGED, markers, K, blobs, poses,
               pairs, rr.COV_MARGIN * oref["cov_spread"])
    far = np.abs(hrows["iters"] - 500) >= 3
    for f in ("iters", "n_pairs", "status"):
        diff = np.flatnonzero(far & (rows[f] != hrows[f]))
        print(f"list {name} K={k}: {f} differs from the host on {len(diff)} of {int(far.sum())} rows "
              f"{[(int(i), int(rows[f][i]), int(hrows[f][i])) for i in diff[:8]]}")
    for f in ("iters", "n_pairs", "status"):
        assert np.array_equal(rows[f][far], hrows[f][far]), f
    check_summary(res, rows, cov)
    assert again["rows"].tobytes() == rows.tobytes() and again["cov"].tobytes() == cov.tobytes()
    assert summary_bytes(again) == summary_bytes(res) == summary_bytes(norows)
    assert norows["rows"].tobytes() == rows.tobytes() and "cov" not in norows


def test_list_empty_and_params():
    markers, K, blobs, poses, pairs, oref = rr.cloud("A")
    sel = np.flatnonzero(oref["n_pairs"] > 0)[:70]
    eng = make_engine(markers, K, 100)
    try:
        res = eng.refine_poses(np.zeros((0, 12)), np.zeros((0, pf.MAX_MARKERS, 2), dtype=np.uint32), blobs=blobs)
        assert res["n"] == 0 and res["best"] == -1 and len(res["rows"]) == 0
        check_summary(res, res["rows"], None)
        # a low cap: nearly every row stops there; without the divergence rule none reverts
        p = pf.default_refine_params()
        p.max_iter = 2
        capped = eng.refine_poses(poses[sel], pairs[sel], blobs=blobs, params=p, want_cov=True)
        at_cap = capped["rows"]["status"] != pf.REFINE_CONVERGED
        assert at_cap.sum() >= 60 and np.all(capped["rows"]["iters"][at_cap] == 2)
        assert np.all(np.isin(capped["rows"]["status"][at_cap], (pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED)))
        hrows, _ = host_ref(markers, K, blobs, poses[sel], pairs[sel], p)
        assert np.array_equal(capped["rows"]["status"], hrows["status"])
        assert np.array_equal(capped["rows"]["iters"], hrows["iters"])
        rev = capped["rows"]["status"] == pf.REFINE_CAP_REVERTED
        assert capped["rows"]["pose"][rev].tobytes() == np.ascontiguousarray(poses[sel][rev]).tobytes()
        check_summary(capped, capped["rows"], capped["cov"])
        p.revert_on_divergence = 0
        kept = eng.refine_poses(poses[sel], pairs[sel], blobs=blobs, params=p)
        assert np.all(kept["rows"]["status"][at_cap] == pf.REFINE_CAP_KEPT) and kept["n_cap_reverted"] == 0
        assert np.array_equal(kept["rows"]["status"] == pf.REFINE_CONVERGED, ~at_cap)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------ CLOUD
def stream_at_scene(name, N):
    """One frame of the synthetic stream whose truth pose and blobs are rr.scene(name)'s, and its prior."""
    M, B, heavy = rr.CONFIGS[name]
    cfg = syn.StreamConfig(name, M=M, B=B, N=N, heavy=heavy)
    st = syn.make_stream(cfg, 2, t0=rr.SCENE_T - cfg.dt)
    return st, st.prior(N)


def stepped_engine(name, N, state):
    st, prior = stream_at_scene(name, N)
    if state != pf.STATE_F64:
        prior = prior.astype(np.float32).astype(np.float64)
    eng = make_engine(st.markers, st.K, N, state, prior)
    fr = st.frames[0]
    out = eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=11,
                                  frame_idx=0))
    return eng, st, out


@pytest.mark.parametrize("n", [300, 2048])
@pytest.mark.parametrize("name", ["B", "A", "C"])
@pytest.mark.parametrize("state", ["f64", "f32", "f16"])
def test_cloud_against_oracle(state, name, n):
    eng, st, _ = stepped_engine(name, n, STATES[state])
    blobs = st.frames[0].blobs
    try:
        for which, wname in ((pf.ASSOC_PROPAGATED, "propagated"), (pf.ASSOC_POSTERIOR, "posterior")):
            tag = f"cloud {state} {name} N={n} {wname}"
            poses = eng.get_particles(which)
            pairs, n_corr = eng.get_pairs(which, blobs=blobs)
            oref = rr.oracle_refine(st.markers, st.K, blobs, poses, pairs)
            res = eng.refine_cloud(which, blobs=blobs, want_cov=True)
            rows, cov = res["rows"], res["cov"]
            assert len(rows) == n and np.array_equal(rows["n_pairs"], n_corr), tag
            print(f"{tag}: oracle under +-1 ulp: cov spread {oref['cov_spread']:.3e}, pose spread "
                  f"{oref['pose_spread_determined']:.3e} m (>= 3 pairs) / {oref['pose_spread_undetermined']:.3e} m (1-2 pairs)")
            rr.compare(tag, rows, cov, oref, oref["iters"] < rr.ORC_CAP, st.markers, st.K, blobs, poses, pairs,
                       rr.COV_MARGIN * oref["cov_spread"])
            check_summary(res, rows, cov)
            # ranges: one particle in the middle, and the summary alone
            one = eng.refine_cloud(which, blobs=blobs, first=37, count=1, want_cov=True)
            assert one["rows"].tobytes() == rows[37:38].tobytes() and one["cov"].tobytes() == cov[37:38].tobytes(), tag
            none = eng.refine_cloud(which, blobs=blobs, count=0)
            assert len(none["rows"]) == 0
            # repeated calls: the same bytes
            again = eng.refine_cloud(which, blobs=blobs, want_cov=True)
            assert again["rows"].tobytes() == rows.tobytes() and again["cov"].tobytes() == cov.tobytes(), tag
            assert summary_bytes(res) == summary_bytes(one) == summary_bytes(none) == summary_bytes(again), tag
            # the particles and their pairs are as before
            assert np.array_equal(eng.get_particles(which), poses), tag
    finally:
        eng.close()


def test_frame_state_untouched():
    """A step taken after refine calls gives the record and the particles of a twin engine that never refined."""
    recs = []
    for refine in (True, False):
        eng, st, _ = stepped_engine("A", 2048, pf.STATE_F32)
        try:
            if refine:
                blobs = st.frames[0].blobs
                eng.refine_cloud(pf.ASSOC_PROPAGATED, blobs=blobs)
                eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=blobs, want_cov=True)
                p = eng.get_particles(1)[:3]
                eng.refine_poses(p, eng.get_pairs(1, blobs=blobs, count=3)[0], blobs=blobs)
            fr = st.frames[1]
            out = eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                          seed=12, frame_idx=1))
            recs.append((bytes(out), eng.get_particles(0).tobytes(), eng.get_particles(1).tobytes()))
        finally:
            eng.close()
    assert recs[0] == recs[1]


def test_bank_frame_equals_host_list():
    eng, st, _ = stepped_engine("A", 300, pf.STATE_F32)
    blobs = st.frames[0].blobs
    try:
        eng.stage_blob_bank([st.frames[1].blobs, blobs])
        for which in (pf.ASSOC_PROPAGATED, pf.ASSOC_POSTERIOR):
            a = eng.refine_cloud(which, blobs=blobs, want_cov=True)
            b = eng.refine_cloud(which, bank_frame=1, want_cov=True)
            assert a["rows"].tobytes() == b["rows"].tobytes() and a["cov"].tobytes() == b["cov"].tobytes()
            assert summary_bytes(a) == summary_bytes(b)
        poses = eng.get_particles(1)[:65]
        pairs = eng.get_pairs(1, blobs=blobs, count=65)[0]
        a = eng.refine_poses(poses, pairs, blobs=blobs, want_cov=True)
        b = eng.refine_poses(poses, pairs, bank_frame=1, want_cov=True)
        assert a["rows"].tobytes() == b["rows"].tobytes() and a["cov"].tobytes() == b["cov"].tobytes()
        assert summary_bytes(a) == summary_bytes(b)
    finally:
        eng.close()


def test_errors():
    markers, K, blobs, poses, pairs, oref = rr.cloud("A")
    sel = np.flatnonzero(oref["n_pairs"] == 5)[:4]
    poses, pairs = poses[sel], pairs[sel]
    lib = pf.load()

    def code(fn):
        with pytest.raises(pf.PFError) as e:
            fn()
        return e.value.code

    def prm(**kw):
        p = pf.default_refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    eng = pf.Engine(device=0, max_particles=8, max_blobs=32)
    try:
        # no model yet
        assert code(lambda: eng.refine_poses(poses, pairs, blobs=blobs)) == pf.E_STATE
        eng.set_model(markers, K)
        # CLOUD without a particle set, PROPAGATED before the first step
        assert code(lambda: eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=blobs, count=0)) == pf.E_STATE
        eng.set_prior(np.concatenate([poses, poses]))
        assert code(lambda: eng.refine_cloud(pf.ASSOC_PROPAGATED, blobs=blobs)) == pf.E_STATE
        eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=blobs)
        eng.refine_poses(poses, pairs, blobs=blobs)
        # arguments
        ai, keep = eng._assoc_in(blobs, -1)
        out = pf.RefineOut()
        u32 = ctypes.POINTER(ctypes.c_uint32)
        pp = np.ascontiguousarray(poses).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        cp = np.ascontiguousarray(pairs).ctypes.data_as(u32)
        assert lib.pfmpe_refine_poses(eng.ctx, ctypes.byref(ai), None, pp, cp, 4, None, None, None) == pf.E_ARG
        assert lib.pfmpe_refine_poses(eng.ctx, None, None, pp, cp, 4, ctypes.byref(out), None, None) == pf.E_ARG
        assert lib.pfmpe_refine_poses(eng.ctx, ctypes.byref(ai), None, None, cp, 4, ctypes.byref(out), None, None) == pf.E_ARG
        assert lib.pfmpe_refine_poses(eng.ctx, ctypes.byref(ai), None, pp, None, 4, ctypes.byref(out), None, None) == pf.E_ARG
        assert lib.pfmpe_refine_poses(eng.ctx, ctypes.byref(ai), None, pp, cp, -1, ctypes.byref(out), None, None) == pf.E_ARG
        assert lib.pfmpe_refine_poses(eng.ctx, ctypes.byref(ai), None, None, None, 0, ctypes.byref(out), None, None) == pf.OK
        assert lib.pfmpe_refine_cloud(eng.ctx, 1, ctypes.byref(ai), None, 0, 0, None, None, None) == pf.E_ARG
        assert lib.pfmpe_refine_cloud(eng.ctx, 1, None, None, 0, 0, ctypes.byref(out), None, None) == pf.E_ARG
        bad = pairs.copy()
        bad[1, 0, 0] = len(markers) + 1
        assert code(lambda: eng.refine_poses(poses, bad, blobs=blobs)) == pf.E_ARG
        bad = pairs.copy()
        bad[2, 1, 1] = len(blobs) + 1
        assert code(lambda: eng.refine_poses(poses, bad, blobs=blobs)) == pf.E_ARG
        nan = poses.copy()
        nan[3, 7] = np.nan
        assert code(lambda: eng.refine_poses(nan, pairs, blobs=blobs)) == pf.E_ARG
        for which in (-1, 2):
            assert code(lambda: eng.refine_cloud(which, blobs=blobs)) == pf.E_ARG
        assert code(lambda: eng.refine_cloud(1, blobs=blobs, first=-1, count=1)) == pf.E_ARG
        assert code(lambda: eng.refine_cloud(1, blobs=blobs, first=0, count=-1)) == pf.E_ARG
        assert code(lambda: eng.refine_cloud(1, blobs=blobs, first=5, count=4)) == pf.E_ARG
        assert code(lambda: eng.refine_cloud(1, bank_frame=0)) == pf.E_ARG  # no bank staged
        for p in (prm(max_iter=0), prm(max_iter=10001), prm(converged=-1.0), prm(converged=float("nan"))):
            assert code(lambda: eng.refine_poses(poses, pairs, blobs=blobs, params=p)) == pf.E_ARG
            assert code(lambda: eng.refine_cloud(1, blobs=blobs, params=p)) == pf.E_ARG
        # capacity
        many = np.zeros((33, 2))
        assert code(lambda: eng.refine_cloud(1, blobs=many)) == pf.E_CAP
        assert code(lambda: eng.refine_poses(poses, pairs, blobs=many)) == pf.E_CAP
        nine = np.concatenate([poses, poses, poses[:1]])
        assert code(lambda: eng.refine_poses(nine, np.concatenate([pairs, pairs, pairs[:1]]), blobs=blobs)) == pf.E_CAP
        # the context still works
        assert eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=blobs)["n"] == 8
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ closed loop
class Tracker:
    """The host state PoseEstimator keeps between frames (PE:995-1010, 2010-2021)."""

    def __init__(self, st):
        f0 = st.frames[0]
        self.t_cur = f0.time - f0.dt
        self.t_prev = self.t_cur - f0.dt
        self.cur = syn.to12(syn.truth_pose(self.t_cur))
        self.prev = syn.to12(syn.truth_pose(self.t_prev))

    def predict(self, t):
        return orc.predict_pose(self.prev, self.cur, self.t_prev, self.t_cur, t)

    def update(self, refined, t):
        self.prev, self.cur = self.cur, refined
        if t - self.t_cur > 0.001 or t < self.t_cur:
            self.t_prev, self.t_cur = self.t_cur, t


def test_closed_loop_c1_refined_on_device():
    """C1 over 30 frames, fp64 state and the reference RNG: the engine loop refines its winner with refine_poses, the
    oracle loop with orc.optimise_pose.  Every frame's discrete step outputs identical, the published poses within
    1e-9.  A frame where the oracle's Gauss-Newton stopped at its cap is exempt (its outcome there is decided by
    rounding noise) and both loops go on from the oracle's pose; at most 5 % of the frames."""
    cfg = syn.CONFIGS["C1"]
    n_frames = 30
    st = syn.make_stream(cfg, n_frames)
    prior = st.prior()
    eng = make_engine(st.markers, st.K, cfg.N, pf.STATE_F64, prior, pf.RNG_REFERENCE)
    op = orc.make_params(rng_mode=pf.RNG_REFERENCE, fast_search=1)
    te, to = Tracker(st), Tracker(st)
    o_prior = prior
    exempt, worst = [], 0.0
    try:
        for f, fr in enumerate(st.frames):
            seed = 900 + f
            pm, pp = te.predict(fr.time)
            rec = eng.step(eng.make_frame(te.cur, pp, pm, blobs=fr.blobs, dt=fr.time - te.t_cur, seed=seed, frame_idx=f))
            out = rec.as_dict()
            pm_o, pp_o = to.predict(fr.time)
            ref, arr = orc.pf_step(st.markers, st.K, op, o_prior, to.cur, pp_o, pm_o, fr.blobs, dt=fr.time - to.t_cur,
                                   seed=seed, frame_idx=f)
            for k in ("iters", "kept_iter", "accepted", "most_likely_idx", "winner_idx", "n_corr", "flag_fail"):
                assert out[k] == ref[k], (f, k, out[k], ref[k])
            assert np.array_equal(out["pairs"], ref["pairs"]), f
            assert out["accepted"] == 1
            corr = np.array(rec.corr, dtype=np.uint32).reshape(1, pf.MAX_MARKERS, 2)
            res = eng.refine_poses(out["winner_pose"], corr, blobs=fr.blobs, want_cov=True)
            pe = res["rows"]["pose"][0].copy()
            po, cov_o, it = orc.optimise_pose(st.markers, st.K, fr.blobs, ref["pairs"], ref["winner_pose"])
            assert res["best"] == 0 and res["rows"]["n_pairs"][0] == out["n_corr"]
            if it >= rr.ORC_CAP:
                exempt.append(f)
                pe = po.copy()
            else:
                d = float(np.abs(pe - po).max())
                worst = max(worst, d)
                assert d <= 1e-9, (f, d)
            te.update(pe, fr.time)
            to.update(po, fr.time)
            o_prior = arr["resampled"]
    finally:
        eng.close()
    print(f"closed loop C1: {n_frames} frames, exempt (oracle at its cap) {exempt}, max pose difference {worst:.3e}")
    assert len(exempt) <= 0.05 * n_frames
