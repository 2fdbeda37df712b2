"""The Gauss-Newton refinement on the device over the case list of gn_cases.py, and across the chunk seam.

DESIGN §4.13 states that pfmpe_host_optimise_pose is a lane of the kernel to the bit.  Here that is asserted: every row
and covariance of every case, the rows with non-finite results included, must be the host's bytes (the host against
the oracle: test_gn_envelope_host.py); every summary must be numpy's over the rows; one refine_multi batch of six
models with per-stream parameters must equal its single calls; and a call of 65,536 + 300 hypotheses, which
pfmpe_refine_poses and pfmpe_refine_cloud process in two chunks, must give the rows of the tiled host reference and the
summary of numpy over all rows, in three arrangements of where the best row lies.

The step's tail (pfmpe_step_refine) does not take the list's rows: its pair row is the step winner's, which the
likelihood builds (every LED at most once, finite blobs within tol_PF of a finite projection, K = 1, so no holes, no
non-finite blob, no tie), and a frame that wins with one of the degenerate rows cannot be built from outside.  The
tail runs gn_optimise on the numbers refine_poses gets, and test_gpu_step_refine.py pins it to refine_poses and to
pfmpe_host_step_tail byte for byte; the function itself is covered here through refine_poses.
"""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

import gn_cases as gc
from test_gpu_refine import best_of, check_summary, summary_bytes

pytestmark = pytest.mark.gpu

CHUNK = 65536  # hypotheses per launch of pfmpe_refine_poses / pfmpe_refine_cloud
SEAM_N = CHUNK + 300


def make_engine(markers, K, max_particles=1024, state=pf.STATE_F64):
    eng = pf.Engine(device=0, max_particles=max_particles, state_dtype=state)
    eng.set_model(markers, K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_PHILOX
    eng.set_params(prm)
    return eng


def first_difference(got, want, names=()):
    """Index of the first element whose bytes differ, and the named indices that differ (for the failure message)."""
    g = np.frombuffer(got.tobytes(), dtype=np.uint8).reshape(len(got), -1)
    w = np.frombuffer(want.tobytes(), dtype=np.uint8).reshape(len(want), -1)
    diff = np.flatnonzero(np.any(g != w, axis=1))
    return (int(diff[0]) if len(diff) else -1, len(diff), [i for i in names if i in set(diff.tolist())])


def assert_same_bytes(tag, res, hrows, hcov, names=()):
    at, n, named = first_difference(res["rows"], hrows, names)
    detail = ""
    if at >= 0:
        detail = f"device {res['rows'][at]} host {hrows[at]}"
    assert at < 0, f"{tag}: {n} rows differ from the host, the first at {at}; of {list(names)}: {named}; {detail}"
    at, n, named = first_difference(res["cov"], hcov, names)
    assert at < 0, f"{tag}: {n} covariances differ from the host, the first at {at}; of {list(names)}: {named}"


# ------------------------------------------------------------------------------------------- every case, LIST
@pytest.mark.parametrize("cid", gc.CASE_IDS)
def test_case_equals_the_host(cid):
    c = gc.case_by_id(cid)
    hrows, hcov = gc.host_rows(c)
    eng = make_engine(c.markers, c.K)
    try:
        res = eng.refine_poses(c.poses, c.pairs, blobs=c.blobs, params=gc.params(c), want_cov=True)
    finally:
        eng.close()
    assert_same_bytes(cid, res, hrows, hcov)
    check_summary(res, hrows, hcov)
    if cid == "ties":
        assert res["best"] == c.note["best"]
    if cid == "degenerate":
        assert res["best"] in set(c.note["all16"].tolist())


# ------------------------------------------------------------------------------------------------- the batch
MULTI_IDS = ["M1-light", "M3-light", "M6-heavy", "M9-light", "M13-heavy", "M16-light"]
MULTI_PARAMS = [None, "it3", "conv1e-6", "it3-keep", "it10000", "conv0"]
MULTI_ROWS = [1, 65, 300, 7, 64, 130]


def test_refine_multi_equals_the_single_calls():
    """Streams of 1, 3, 6, 9, 13 and 16 LEDs, each with parameters of its own from the list, as one batch."""
    cases = [gc.case_by_id(cid) for cid in MULTI_IDS]
    assert [len(c.markers) for c in cases] == [1, 3, 6, 9, 13, 16]
    prms = []
    for name in MULTI_PARAMS:
        p = pf.default_refine_params()
        for k, v in (gc.PARAM_SETS[name] if name else {}).items():
            setattr(p, k, v)
        prms.append(p)
    engs = [make_engine(c.markers, c.K) for c in cases]
    try:
        poses, pairs, blobs = [], [], []
        for c, n in zip(cases, MULTI_ROWS):
            sel = np.flatnonzero(np.count_nonzero(c.pairs[:, :, 1], axis=1) > 0)[:n]
            assert len(sel) == n
            poses.append(c.poses[sel].copy())
            pairs.append(c.pairs[sel].copy())
            blobs.append(c.blobs.copy())
        ref = [engs[s].refine_poses(poses[s], pairs[s], blobs=blobs[s], params=prms[s], want_cov=True)
               for s in range(len(cases))]
        got = pf.Engine.refine_multi(engs, poses, pairs, blobs, params=prms, want_rows=True, want_cov=True)
    finally:
        for e in engs:
            e.close()
    for s, (g, r) in enumerate(zip(got, ref)):
        assert g["rows"].tobytes() == r["rows"].tobytes(), s
        assert g["cov"].tobytes() == r["cov"].tobytes(), s
        assert summary_bytes(g) == summary_bytes(r), s
        check_summary(g, g["rows"], g["cov"])
        # and the single call is the host's rows under the stream's own parameters
        c = cases[s]
        sel = np.flatnonzero(np.count_nonzero(c.pairs[:, :, 1], axis=1) > 0)[: MULTI_ROWS[s]]
        for k, i in enumerate(sel[:16]):
            hr, hc = pf.host_optimise_pose(c.markers, c.K, c.blobs, c.pairs[i], c.poses[i], prms[s])
            assert hr.tobytes() == g["rows"][k].tobytes() and hc.tobytes() == g["cov"][k].tobytes(), (s, k)
    assert got[1]["iters_max"] == 3 and got[3]["n_cap_reverted"] == 0


# -------------------------------------------------------------------------------------------- the chunk seam
def seam_inputs(arrangement):
    """(poses, pairs, host rows, host cov) of SEAM_N hypotheses: M5-light's 700 tiled, then arranged."""
    c = gc.bucket_case_5()
    hrows, hcov = gc.host_rows(c)
    blank = gc.Case("M5-light-unpaired", c.markers, c.K, c.blobs, c.poses, np.zeros_like(c.pairs))
    brows, bcov = gc.host_rows(blank)  # the rows of the same poses without pairs
    base = np.arange(SEAM_N) % len(c.poses)
    paired = np.ones(SEAM_N, dtype=bool)
    b = best_of(hrows)
    if arrangement == "best-in-chunk-2":  # chunk 1 all without pairs
        paired[:CHUNK] = False
    elif arrangement == "tie-across-the-seam":  # of the best row's copies only two keep their pairs, one in each chunk
        copies = np.flatnonzero(base == b)
        first = int(copies[copies < CHUNK].max())
        if np.any(copies >= CHUNK):
            second = int(copies[copies >= CHUNK].min())
        else:  # the tile does not reach b in chunk 2: the last hypothesis becomes a copy
            second = SEAM_N - 1
            base[second] = b
        paired[base == b] = False
        paired[[first, second]] = True
    elif arrangement == "best-in-chunk-1":  # chunk 2 without the best row
        paired[(base == b) & (np.arange(SEAM_N) >= CHUNK)] = False
    else:
        raise KeyError(arrangement)
    poses = c.poses[base]
    pairs = c.pairs[base].copy()
    pairs[~paired] = 0
    rows, cov = hrows[base].copy(), hcov[base].copy()
    rows[~paired], cov[~paired] = brows[base][~paired], bcov[base][~paired]
    return c, poses, pairs, rows, cov


def numpy_summary(rows):
    return {"n": len(rows), "n_with_pairs": int(np.count_nonzero(rows["n_pairs"] > 0)),
            "n_converged": int(np.count_nonzero(rows["status"] == pf.REFINE_CONVERGED)),
            "n_cap_kept": int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_KEPT)),
            "n_cap_reverted": int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_REVERTED)),
            "iters_total": int(rows["iters"].astype(np.int64).sum()), "iters_max": int(rows["iters"].max()),
            "best": best_of(rows)}


@pytest.fixture(scope="module")
def seam_engine():
    c = gc.bucket_case_5()
    eng = make_engine(c.markers, c.K, max_particles=SEAM_N)
    yield eng
    eng.close()


@pytest.mark.parametrize("arrangement", ["best-in-chunk-2", "tie-across-the-seam", "best-in-chunk-1"])
def test_chunk_seam(seam_engine, arrangement):
    c, poses, pairs, hrows, hcov = seam_inputs(arrangement)
    assert len(poses) == SEAM_N
    want = numpy_summary(hrows)
    if arrangement == "best-in-chunk-2":
        assert want["best"] >= CHUNK and not np.any(hrows["n_pairs"][:CHUNK])
    elif arrangement == "tie-across-the-seam":
        twins = np.flatnonzero((hrows["n_pairs"] == hrows["n_pairs"][want["best"]]) &
                               (hrows["rms_after"] == hrows["rms_after"][want["best"]]))
        assert want["best"] < CHUNK and twins.min() == want["best"] and twins.max() >= CHUNK
    else:
        assert want["best"] < CHUNK and np.any(hrows["n_pairs"][CHUNK:] > 0)
    res = seam_engine.refine_poses(poses, pairs, blobs=c.blobs, want_cov=True)
    again = seam_engine.refine_poses(poses, pairs, blobs=c.blobs, want_cov=True)
    assert_same_bytes(arrangement, res, hrows, hcov, names=(CHUNK - 1, CHUNK, SEAM_N - 1))
    for k, v in want.items():
        assert res[k] == v, (arrangement, k, res[k], v)
    assert res["best_row"].tobytes() == res["rows"][res["best"]].tobytes()
    assert res["best_cov"].tobytes() == res["cov"][res["best"]].tobytes()
    check_summary(res, hrows, hcov)
    assert again["rows"].tobytes() == res["rows"].tobytes() and again["cov"].tobytes() == res["cov"].tobytes()
    assert summary_bytes(again) == summary_bytes(res)


def test_refine_cloud_across_the_seam():
    """fp32 state, N = 65,836, one step, the posterior: rows of a range that straddles nothing but lies in chunk 1's
    tail and chunk 2's head (65,500 .. 65,599) against refine_poses on the same particles and pairs; the summary of
    the range call against the full call's and numpy's over all rows."""
    cfg = syn.StreamConfig("seam", M=5, B=50, N=SEAM_N)
    st = syn.make_stream(cfg, 1)
    fr = st.frames[0]
    eng = make_engine(st.markers, st.K, max_particles=SEAM_N, state=pf.STATE_F32)
    try:
        eng.set_prior(st.prior(SEAM_N).astype(np.float32).astype(np.float64))
        eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=21,
                                frame_idx=0))
        first, count = 65500, 100
        full = eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=fr.blobs, want_cov=True)
        part = eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=fr.blobs, first=first, count=count, want_cov=True)
        poses = eng.get_particles(pf.ASSOC_POSTERIOR)
        pairs, n_corr = eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=fr.blobs)
        lst = eng.refine_poses(poses[first:first + count], pairs[first:first + count], blobs=fr.blobs, want_cov=True)
        whole = eng.refine_poses(poses, pairs, blobs=fr.blobs, want_cov=True)
    finally:
        eng.close()
    assert len(full["rows"]) == SEAM_N and len(part["rows"]) == count
    assert part["rows"].tobytes() == lst["rows"].tobytes() and part["cov"].tobytes() == lst["cov"].tobytes()
    assert part["rows"].tobytes() == full["rows"][first:first + count].tobytes()
    assert part["cov"].tobytes() == full["cov"][first:first + count].tobytes()
    assert summary_bytes(part) == summary_bytes(full)
    at, n, named = first_difference(full["rows"], whole["rows"], (CHUNK - 1, CHUNK, SEAM_N - 1))
    assert at < 0, f"refine_cloud against refine_poses: {n} rows differ, the first at {at}; {named}"
    assert full["cov"].tobytes() == whole["cov"].tobytes() and summary_bytes(full) == summary_bytes(whole)
    assert np.array_equal(full["rows"]["n_pairs"], n_corr)
    want = numpy_summary(full["rows"])
    for k, v in want.items():
        assert full[k] == v, (k, full[k], v)
    check_summary(full, full["rows"], full["cov"])
    assert np.any(full["rows"]["n_pairs"][:CHUNK] > 0) and np.any(full["rows"]["n_pairs"][CHUNK:] > 0)
