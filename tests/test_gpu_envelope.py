"""Step parity over the input envelope: every marker bucket, blob-table form and frame predicate against the oracle.

The host picks the step's code variant from the model (marker bucket: exact-5, 8, 12 or 16 slots), the blobs (x-bucket
count, fine / coarse cell grid or none, table size in LDS), the parameters (small-angle bound, tol_PF) and the frame
(camMoveInv, K, non-finite blobs, B < M).  tests/envelope_cases.py lists the cases; here each runs at N = 700 in the
frame shapes named below, next to an unpruned engine that must give the same record and weights bit for bit, and is
held against orc.pf_step by the project's own rules:

  * fp64 state: assert_exact (test_gpu_parity.py);
  * fp32 state: check_fp32_frame (the body of test_fp32_tolerance), the oracle starting from the engine's own prior;
    a frame of more than one iteration may keep another iteration than the oracle on a near tie, so its weights and
    poses are compared at the engine's own kept iteration (orc.pf_sample) and its best weight within 2e-3;
  * fp16 state: the rules of test_fp16_state.

tests/test_envelope_inputs.py shows from the oracle alone that no case sits near the tol_PF gate (the cap of three
flipped particles is a condition on the inputs) and that each does what it is there for.  Run with -s for the observed
(case, state, shape, pass, grid) rows and the largest errors.
"""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from oracle import pforacle as orc

import envelope_cases as ec
from test_gpu_multi import _check_batch
from test_gpu_parity import assert_exact, check_fp32_frame, make_engine, rotation_angle, step_both

pytestmark = pytest.mark.gpu

N = ec.N
F64, F32, F16 = pf.STATE_F64, pf.STATE_F32, pf.STATE_F16
STATE_NAME = {F64: "f64", F32: "f32", F16: "f16"}
# every frame shape: (OPT_FUSED, OPT_DIAG)
SHAPES = {
    "flat": (2, 0),      # one launch, flat hand-offs
    "tree": (1, 0),      # one launch, tree hand-offs
    "two": (0, 0),       # two launches
    "stream": (0, pf.DIAG_FORCE_STREAM),
    "stream-nopk": (0, pf.DIAG_FORCE_STREAM | pf.DIAG_NO_PK),
}
EVERY = list(SHAPES)
FUSED3 = ["flat", "tree", "two"]
SHAPE_NAME = {pf.SHAPE_TWO_LAUNCH: "two-launch", pf.SHAPE_FRAME: "k_frame", pf.SHAPE_FRAME2: "k_frame2"}
PASS_NAME = {pf.WEIGH_BLOCKS: "blocks", pf.WEIGH_STREAM: "stream", pf.WEIGH_PK: "pk", -1: "-"}

ERR = {}  # state name -> [largest weight error among unflipped particles, largest pose entry error, largest angle]


def _note(state, gpu, arr):
    e = ERR.setdefault(STATE_NAME[state], [0.0, 0.0, 0.0])
    dw = np.abs(gpu["weights"] - arr["weights"])
    ok = dw <= 2e-3
    e[0] = max(e[0], float(dw[ok].max()) if ok.any() else 0.0)
    dp = np.abs(gpu["propagated"] - arr["propagated"])
    e[1] = max(e[1], float(dp.max()))
    n = int(np.argmax(dp.max(axis=1)))
    e[2] = max(e[2], rotation_angle(gpu["propagated"][n].reshape(3, 4)[:, :3], arr["propagated"][n].reshape(3, 4)[:, :3]))


def _bits(v):
    return np.ascontiguousarray(v).tobytes()


def _at_kept_iteration(inp, out, prior_used):
    """The oracle's propagated set and weights of the engine's own kept iteration (Philox)."""
    p, w = orc.pf_sample(inp.markers, inp.K, ec.orc_params(inp, pf.RNG_PHILOX), np.arange(N), prior_used, inp.cur,
                         inp.pred, inp.predm, inp.blobs, out["kept_iter"], it_since_init=inp.it, dt=inp.dt,
                         seed=inp.seed, frame_idx=inp.frame_idx, cam_move_inv=inp.cam, downgrade=inp.downgrade)
    return {"weights": w, "propagated": p}


def _check(inp, state, rng, prm, out, gpu, ref, arr, prior_used):
    if state == F64:
        assert_exact(out, gpu, ref, arr, N)
        _note(state, gpu, arr)
        return
    if ref["iters"] > 1:
        assert out["iters"] == ref["iters"]
        assert abs(out["highest_prob"] - ref["highest_prob"]) <= 2e-3
        arr = _at_kept_iteration(inp, out, prior_used)
    if state == F32:
        check_fp32_frame(out, gpu, ref, arr, N, rng, inp.seed, inp.frame_idx, inp.markers, inp.K, inp.blobs, prm,
                         downgrade=inp.downgrade, refine=False)
    else:  # the rules of test_fp16_state
        assert out["accepted"] == ref["accepted"]
        dw = np.abs(gpu["weights"] - arr["weights"])
        assert np.sum(dw > 2e-3) <= max(3, N // 1000), np.sort(dw)[-10:]
        if out["resampled"]:
            c = gpu["counts"].astype(np.int64)
            assert c.sum() == N
            src = np.repeat(np.arange(N), c)
            err = np.abs(gpu["resampled"] - gpu["propagated"][src])
            delta = np.abs(gpu["propagated"][src] - np.asarray(inp.cur).reshape(1, 12))
            assert np.all(err <= delta * 2.0 ** -10 + 1e-7), err.max()
    _note(state, gpu, arr)


def _expected_pass(inp, state, rng, shape, grid):
    """The weighing pass of a two-launch frame (pfmpe_seq.hpp pk_eligible)."""
    pk = state != F64 and rng == pf.RNG_PHILOX and shape != "stream-nopk" and inp.pk_ok and grid == 1
    return pf.WEIGH_PK if pk else pf.WEIGH_STREAM


def run_case(frames, state, rng, shapes, rows=None):
    """frames (one model, one parameter set) in each shape: a pruned engine against the oracle and, bit for bit,
    against an unpruned engine.  Returns the observed (frame, state, shape, last shape, pass, grid) rows."""
    rows = [] if rows is None else rows
    f0 = frames[0]
    prm = ec.params(f0, rng)
    for shape in shapes:
        fused, diag = SHAPES[shape]
        engs = []
        try:
            for prune in (True, False):
                e = make_engine(N, f0.markers, f0.K, state, rng, prune=prune, downgrade=f0.downgrade, params=prm, fused=fused)
                e.set_option(pf.OPT_DIAG, diag)
                engs.append(e)
            pruned, brute = engs
            for inp in frames:
                for e in engs:
                    e.set_prior(ec.prior())
                prior_used = ec.prior() if state == F64 else pruned.get_particles(1)
                ref = ec.oracle_cached(inp, rng, prior_used, STATE_NAME[state])
                out, gpu, ref, arr = step_both(pruned, prm, inp.markers, inp.K, prior_used, inp.cur, inp.pred, inp.predm,
                                               inp.blobs, seed=inp.seed, frame_idx=inp.frame_idx, it=inp.it, dt=inp.dt,
                                               force_iters=inp.force_iters, cam=inp.cam, downgrade=inp.downgrade, ref=ref)
                last, wpass, grid = (pruned.info(k) for k in (pf.INFO_LAST_SHAPE, pf.INFO_LAST_WEIGH_PASS, pf.INFO_LAST_GRID))
                two = last == pf.SHAPE_TWO_LAUNCH
                rows.append((inp.name, STATE_NAME[state], shape, SHAPE_NAME[last], PASS_NAME[wpass if two else -1], grid))
                if fused == 0:
                    assert two
                    assert wpass == _expected_pass(inp, state, rng, shape, grid), rows[-1]
                    if shape == "stream" and state != F64 and rng == pf.RNG_PHILOX and "pass" in inp.want:
                        assert wpass == inp.want["pass"], rows[-1]
                if state != F64 and "grid" in inp.want:
                    assert grid == inp.want["grid"], rows[-1]
                # pruning changes no bit of the record or the weights
                other = brute.step(brute.make_frame(inp.cur, inp.pred, inp.predm, blobs=inp.blobs, dt=inp.dt, seed=inp.seed,
                                                    frame_idx=inp.frame_idx, it_since_init=inp.it,
                                                    force_iters=inp.force_iters, cam_move_inv=inp.cam)).as_dict()
                for k, v in out.items():
                    assert _bits(v) == _bits(other[k]), (rows[-1], k)
                assert _bits(gpu["weights"]) == _bits(brute.get_weights()), rows[-1]
                if inp.want.get("zero_weights"):
                    assert np.all(gpu["weights"] == 0.0) and _bits(gpu["weights"]) == _bits(np.zeros(N))
                _check(inp, state, rng, prm, out, gpu, ref, arr, prior_used)
        finally:
            for e in engs:
                e.close()
    for r in rows:
        print("envelope:", *r)
    print("envelope errors (weight, pose entry, angle):", {k: [f"{x:.3g}" for x in v] for k, v in ERR.items()})
    return rows


# ------------------------------------------------------------------------------------------ 1. marker counts
@pytest.mark.parametrize("rng", [pf.RNG_REFERENCE, pf.RNG_PHILOX], ids=["ref", "philox"])
@pytest.mark.parametrize("case", ec.MARKER_CASES, ids=ec.marker_id)
def test_marker_counts_fp64(case, rng):
    run_case(ec.marker_case(*case), F64, rng, FUSED3)


@pytest.mark.parametrize("case", ec.MARKER_CASES, ids=ec.marker_id)
def test_marker_counts_fp32(case):
    run_case(ec.marker_case(*case), F32, pf.RNG_PHILOX, EVERY)


@pytest.mark.parametrize("case", [c for c in ec.MARKER_CASES if c[0] in ec.FP16_MS], ids=ec.marker_id)
def test_marker_counts_fp16(case):
    run_case(ec.marker_case(*case), F16, pf.RNG_PHILOX, ["stream"])


@pytest.mark.parametrize("state,rng", [(F64, pf.RNG_REFERENCE), (F64, pf.RNG_PHILOX), (F32, pf.RNG_PHILOX)],
                         ids=["f64-ref", "f64-philox", "f32"])
@pytest.mark.parametrize("M", ec.EXTRA_MS)
def test_marker_bucket_last_slot_penalties(M, state, rng):
    """Per bucket (8, 12 with a dead slot, 16): LEDs 0 and M-1 downgraded, LED M-1 on LED M-2's blob (the duplicate
    penalty on the last live slot, downgrade bit M-1), B = M - 1 (the sorted score)."""
    run_case(ec.marker_extra(M), state, rng, FUSED3 if state == F64 else EVERY)


@pytest.mark.parametrize("state,rng", [(F64, pf.RNG_REFERENCE), (F32, pf.RNG_PHILOX)], ids=["f64-ref", "f32-philox"])
def test_marker_counts_in_one_batch(state, rng):
    """Streams of 3, 5, 8, 13 and 16 LEDs in one pfmpe_step_multi batch (the 16-slot bucket serves all of them): each
    equals its own pfmpe_step bit for bit."""
    cfgs = [(N, M, max(M, 20), False, "") for M in ec.BATCH_MS]
    _check_batch(state, rng, 2, cfgs)


# -------------------------------------------------------------------------------------------- 2. blob counts
@pytest.mark.parametrize("case", ec.BLOB_CASES, ids=ec.blob_id)
def test_blob_counts_fp32(case):
    run_case(ec.blob_case(*case), F32, pf.RNG_PHILOX, EVERY)


@pytest.mark.parametrize("case", ec.BLOB_CASES, ids=ec.blob_id)
def test_blob_counts_fp64(case):
    run_case(ec.blob_case(*case), F64, pf.RNG_REFERENCE, ["flat", "two"])


def test_blob_counts_deep_fp64():
    """M = 16, B = 1024, twelve forced iterations: the largest table across the noise growth step at iteration 10."""
    rows = run_case(ec.blob_case(16, True, 1024, True), F64, pf.RNG_REFERENCE, ["flat", "two"])
    assert len(rows) == 2


def test_blob_table_forms_are_covered():
    """The fp32 sweep reaches the cell grid at B >= 128 and the x-bucket search (no grid), and the packed passes
    whenever the grid is on for a 5- or 12-LED model with B >= M; nothing here fixes which B takes which form."""
    rows = []
    for M, heavy, B in ec.BLOB_CASES:
        inp = ec.blob_case(M, heavy, B)[0]
        prm = ec.params(inp, pf.RNG_PHILOX)
        eng = make_engine(N, inp.markers, inp.K, F32, pf.RNG_PHILOX, params=prm, fused=0)
        try:
            eng.set_option(pf.OPT_DIAG, pf.DIAG_FORCE_STREAM)
            eng.set_prior(ec.prior())
            eng.step(eng.make_frame(inp.cur, inp.pred, inp.predm, blobs=inp.blobs, dt=inp.dt, seed=inp.seed,
                                    frame_idx=inp.frame_idx, it_since_init=inp.it, force_iters=inp.force_iters))
            rows.append((M, B, eng.info(pf.INFO_LAST_WEIGH_PASS), eng.info(pf.INFO_LAST_GRID)))
        finally:
            eng.close()
    for M, B, wpass, grid in rows:
        print("envelope blob table:", M, B, PASS_NAME[wpass], grid)
        assert wpass == (pf.WEIGH_PK if grid == 1 and M in (5, 12) and B >= M else pf.WEIGH_STREAM), (M, B)
    assert any(grid == 1 and B >= 128 for _, B, _, grid in rows)
    assert any(grid == 0 for _, _, _, grid in rows)
    assert any(wpass == pf.WEIGH_PK for M, _, wpass, _ in rows if M == 5)
    assert any(wpass == pf.WEIGH_PK for M, _, wpass, _ in rows if M == 12)


# ---------------------------------------------------------------------------------------- 3. frame predicates
@pytest.mark.parametrize("case", ec.PRED_CASES, ids=ec.pred_id)
def test_frame_predicates_fp32(case):
    run_case(ec.pred_case(*case), F32, pf.RNG_PHILOX, ["flat", "stream"])


@pytest.mark.parametrize("case", ec.PRED_FP16_CASES, ids=ec.pred_id)
def test_frame_predicates_fp16(case):
    run_case(ec.pred_case(*case), F16, pf.RNG_PHILOX, ["flat", "stream"])


@pytest.mark.parametrize("base", list(ec.BASELINES))
def test_nan_blob_zero_weights_fp64(base):
    """Blob 0 = NaN: every weight exactly 0, 80 iterations, re-initialisation, in fp64 as well."""
    rows = run_case(ec.pred_case(base, "nan0"), F64, pf.RNG_PHILOX, ["flat", "stream"])
    assert len(rows) == 2
