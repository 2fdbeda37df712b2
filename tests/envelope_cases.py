"""Inputs of the step-parity sweep over the input envelope (tests/test_gpu_envelope.py, tests/test_envelope_inputs.py).

The PF step picks its code variant from what the host sees in the model (the marker bucket: exact-5, 8, 12 or 16
slots), the blobs (x-bucket count, fine / coarse cell grid or none, table size), the parameters (small-angle bound,
tol_PF) and the frame (camMoveInv, K, non-finite blobs, B < M).  This module holds one table of cases per switch and
the builders of their inputs; the GPU module runs them against the oracle, the CPU module checks from the oracle alone
that every case does what it is there for and sits away from the tol_PF gate.

Everything runs at N = 700 particles: two full 256-particle blocks and a partial one, particles 0 and 1 (current and
predicted pose) in block 0.  A case is a list of frames sharing one model and one parameter set, so that one engine
serves them; every frame starts from the same prior().
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn
from oracle import pforacle as orc

N = 700
SEED = 4100  # frame seeds: SEED + frame number within the case


@dataclass
class Inp:
    """One frame's inputs."""
    name: str
    markers: np.ndarray
    K: np.ndarray
    blobs: np.ndarray
    cur: np.ndarray
    pred: np.ndarray
    predm: np.ndarray
    dt: float
    it: int = 2
    force_iters: int = 0
    cam: np.ndarray | None = None
    downgrade: np.ndarray | None = None
    prm: dict = field(default_factory=dict)  # fields of pf.Params away from their defaults
    seed: int = SEED
    frame_idx: int = 0
    # the host's packed-pass predicates other than "grid on" hold (pfmpe_seq.hpp pk_eligible): M is 5 or 12, B >= M,
    # blob 0 finite, identity camMoveInv, upper-triangular K with K[8] = 1, every angle draw within the small-angle bound
    pk_ok: bool = False
    want: dict = field(default_factory=dict)  # what the oracle must give (test_envelope_inputs.py)


@functools.lru_cache(maxsize=None)
def _stream(M, B, heavy, blob_seed=0):
    return syn.make_stream(syn.StreamConfig("env", M=M, B=B, N=N, heavy=heavy, seed=blob_seed), 1)


@functools.lru_cache(maxsize=None)
def _prior():
    p = _stream(5, 20, False).prior()
    p.setflags(write=False)
    return p


def prior() -> np.ndarray:
    """The prior of every frame (the trajectory, and with it frame 0's current pose, is the same for every model)."""
    return _prior()


def prior_f32() -> np.ndarray:
    """prior() as an fp32-state engine holds it."""
    return prior().astype(np.float32).astype(np.float64)


def params(inp: Inp, rng_mode: int):
    prm = pf.default_params()
    for k, v in inp.prm.items():
        setattr(prm, k, v)
    prm.rng_mode = rng_mode
    return prm


def orc_params(inp: Inp, rng_mode: int, **over):
    p = params(inp, rng_mode)
    for k, v in over.items():
        setattr(p, k, v)
    return orc.OrcParams(p.tol, p.tol_pf, p.ang_min, p.ang_max, p.trans_min, p.trans_max, p.growth, p.max_iter,
                         p.exit_cap, p.accept_cap, p.rng_mode)


def oracle(inp: Inp, rng_mode: int, prior_rows, **over):
    """orc.pf_step of the frame from prior_rows; over: parameter overrides (the tol_PF shifts of the CPU checks)."""
    return orc.pf_step(inp.markers, inp.K, orc_params(inp, rng_mode, **over), prior_rows, inp.cur, inp.pred, inp.predm,
                       inp.blobs, it_since_init=inp.it, dt=inp.dt, seed=inp.seed, frame_idx=inp.frame_idx,
                       force_iters=inp.force_iters, cam_move_inv=inp.cam, downgrade=inp.downgrade)


_ORACLE = {}


def oracle_cached(inp: Inp, rng_mode: int, prior_rows, tag):
    """oracle() once per (frame, RNG, tag); tag names the prior (the state type that rounded it).  A second caller
    must bring the same prior rows."""
    key = (inp.name, rng_mode, tag)
    hit = _ORACLE.get(key)
    if hit is None:
        ref, arr = oracle(inp, rng_mode, prior_rows)
        hit = _ORACLE[key] = (np.array(prior_rows, copy=True), ref, arr)
    assert np.array_equal(hit[0], prior_rows), key
    return hit[1], hit[2]


def _inp(name, M, B, heavy, blob_seed=0, **kw) -> Inp:
    st = _stream(M, B, heavy, blob_seed)
    fr = st.frames[0]
    kw.setdefault("blobs", fr.blobs)
    return Inp(name=name, markers=st.markers, K=st.K.copy(), cur=np.array(fr.current_pose), pred=np.array(fr.predicted_pose),
               predm=np.array(fr.prediction), dt=fr.dt, **kw)


def true_px(inp: Inp, K=None) -> np.ndarray:
    """Noise-free projections of the markers at the frame's true pose."""
    return syn.project(inp.K if K is None else K, _stream(5, 20, False).frames[0].truth, inp.markers)


# ------------------------------------------------------------------------------------------ 1. marker counts
MARKER_MS = [1, 2, 3, 4, 6, 7, 8, 9, 11, 13, 15, 16]
MARKER_CASES = [(M, False) for M in MARKER_MS] + [(M, True) for M in MARKER_MS if M >= 6]
FP16_MS = [4, 8, 16]
EXTRA_MS = [8, 11, 16]
BATCH_MS = [3, 5, 8, 13, 16]


def marker_id(case):
    return f"M{case[0]}-{'heavy' if case[1] else 'light'}"


@functools.lru_cache(maxsize=None)
def marker_case(M, heavy):
    """A steady frame and an it_since_init = 1 frame (full noise) of an M-LED model: B = max(M, 20) light, 200 heavy."""
    B = 200 if heavy else max(M, 20)
    tag = marker_id((M, heavy))
    if M <= 2:
        want = {"iters": 80, "flag_fail": pf.FLAG_REINIT, "accepted": 0}
    elif M <= 4:
        want = {"iters": 80, "accepted": 1, "resampled": 1}
    else:
        want = {"accepted": 1, "resampled": 1}
    return [_inp(f"{tag}-steady", M, B, heavy, it=2, seed=SEED, want=dict(want)),
            _inp(f"{tag}-it1", M, B, heavy, it=1, seed=SEED + 1, frame_idx=1, want=dict(want))]


@functools.lru_cache(maxsize=None)
def marker_extra(M):
    """The last live slot of a bucket under every penalty at once.  Two LEDs further than tol_PF apart in the image
    never share a blob, so the duplicate penalty needs LED M-1 next to LED M-2: the model's last LED sits 0.5 mm from
    the one before (0.1 px at 2 m) and has no blob of its own, so both claim LED M-2's blob.  The blobs are those of
    LEDs 0..M-2 (B = M - 1: the sorted score), LEDs 0 and M-1 are downgraded."""
    a = _inp(f"M{M}-extra", M, max(M, 20), False)
    a.markers = a.markers.copy()
    a.markers[M - 1] = a.markers[M - 2] + np.array([0.0005, 0.0, 0.0])
    px = true_px(a)
    blobs = px[: M - 1] + np.random.default_rng(70 + M).normal(0.0, 0.3, size=(M - 1, 2))
    blobs[M - 2] = 0.5 * (px[M - 2] + px[M - 1])  # the shared blob: the closest to both of its LEDs
    a.blobs = blobs.astype(np.float32).astype(np.float64)
    dg = np.zeros(M, np.uint8)
    dg[[0, M - 1]] = 1
    a.downgrade = dg
    a.want = {"accepted": 1, "resampled": 1, "duplicate": True}
    return [a]


# -------------------------------------------------------------------------------------------- 2. blob counts
BLOB_MODELS = [(5, False), (12, True), (16, True)]


def blob_counts(M):
    return [1, M - 1, M, 127, 128, 256, 257, 400, 700, 1024]


BLOB_CASES = [(M, heavy, B) for M, heavy in BLOB_MODELS for B in blob_counts(M)]


def blob_id(case):
    return f"M{case[0]}-B{case[2]}"


@functools.lru_cache(maxsize=None)
def blob_case(M, heavy, B, deep=False):
    """One steady frame with B blobs: the reference exit rule up to B = 200, three forced iterations above (the
    oracle's B x M rescans); deep: twelve forced iterations, across the noise growth step at iteration 10."""
    force = 12 if deep else (0 if B <= 200 else 3)
    want = {"iters": force} if force else {}
    return [_inp(f"{blob_id((M, heavy, B))}{'-deep' if deep else ''}", M, B, heavy, force_iters=force,
                 pk_ok=(M in (5, 12) and B >= M), want=want)]


# ---------------------------------------------------------------------------------------- 3. frame predicates
BASELINES = {"m5": (5, 50, False), "m12": (12, 200, True)}
CAM_MOTION = syn.to12(syn.se3_exp([0.002, -0.001, 0.003, 0.001, 0.0005, -0.002]))


def _far_blobs(inp: Inp, k: int):
    """The blobs with one that is no LED's (the farthest from every true projection) swapped into place k."""
    b = inp.blobs.copy()
    d = np.min(np.linalg.norm(b[:, None, :] - true_px(inp)[None, :, :], axis=2), axis=1)
    j = int(np.argmax(d))
    b[[k, j]] = b[[j, k]]
    return b


def _through(inp: Inp, K2):
    """The frame seen through K2: the blobs mapped by the homography K2 K^-1, like the LEDs' projections."""
    h = (K2 @ np.linalg.inv(inp.K) @ np.column_stack([inp.blobs, np.ones(len(inp.blobs))]).T).T
    inp.blobs = (h[:, :2] / h[:, 2:3]).astype(np.float32).astype(np.float64)
    inp.K = K2
    return inp


def _angles(a):
    return {"ang_min": -a, "ang_max": a}


def _predicate(base, name):
    M, B, heavy = BASELINES[base]
    nm = f"{base}-{name}"
    mk = functools.partial(_inp, nm, M, B, heavy)
    stream, pk = pf.WEIGH_STREAM, pf.WEIGH_PK
    if name == "base":
        return mk(pk_ok=True, want={"pass": pk, "accepted": 1})
    # a. angle noise +-a: the host's small-angle bound a * 1.175 <= 0.999 * 0.03 flips at a = 0.025506...
    if name == "ang0.0255":
        return mk(it=1, prm=_angles(0.0255), pk_ok=True, want={"pass": pk})
    if name == "ang0.0256":
        return mk(it=1, prm=_angles(0.0256), want={"pass": stream})
    if name == "ang0.3-force25":  # draws on both sides of the 0.25 rad split in one wave, and the growth steps
        return mk(it=1, prm=_angles(0.3), force_iters=25, want={"pass": stream, "iters": 25})
    if name == "ang1.0-it1":  # sincosf
        return mk(it=1, prm=_angles(1.0), want={"pass": stream})
    if name == "ang1.0-it2":  # scaled by 0.2: the long polynomial
        return mk(it=2, prm=_angles(1.0), want={"pass": stream})
    if name == "neg-growth":  # the largest draw is at iteration 0: a = 0.032 is outside the bound, 0.032 * 0.95 inside
        return mk(it=1, prm=dict(_angles(0.032), growth=-0.025), force_iters=25, want={"pass": stream, "iters": 25})
    # b. camMoveInv
    if name == "cam":
        return mk(it=2, cam=CAM_MOTION, want={"pass": stream, "accepted": 1})
    # c. K
    if name == "K2":  # the same image through 2 K (K[8] = 2): the general K * pose
        a = mk(want={"pass": stream, "accepted": 1})
        a.K = 2.0 * a.K
        return a
    if name == "Krot":  # K Rx(0.01) Ry(-0.02): a full matrix, the blobs mapped through the same homography
        a = mk(want={"pass": stream, "accepted": 1})
        return _through(a, a.K @ syn.rot_x(0.01) @ syn.rot_y(-0.02))
    if name == "Kskew":  # stays upper-triangular: the packed pass with a skew term
        a = mk(pk_ok=True, want={"pass": pk, "accepted": 1})
        K2 = a.K.copy()
        K2[0, 1] = 0.7
        return _through(a, K2)
    # d. non-finite blobs
    if name == "nan0":
        a = mk(want={"pass": stream, "grid": 0, "iters": 80, "flag_fail": pf.FLAG_REINIT, "zero_weights": True})
        a.blobs = a.blobs.copy()
        a.blobs[0] = np.nan
        return a
    if name in ("inf0", "nan7"):
        a = mk(want={"pass": stream, "grid": 0, "accepted": 1, "same_pairs_as_base": True})
        k = 0 if name == "inf0" else 7
        a.blobs = _far_blobs(a, k)
        a.blobs[k, 0 if name == "inf0" else 1] = np.inf if name == "inf0" else np.nan
        return a
    # e. B = M - 1, LEDs 0 and M-1 downgraded
    if name == "fewer-blobs":
        a = _inp(nm, M, M - 1, False, want={"pass": stream, "accepted": 1})
        dg = np.zeros(M, np.uint8)
        dg[[0, M - 1]] = 1
        a.downgrade = dg
        return a
    # f. tol_PF away from 4 (tol stays 5)
    if name.startswith("tolpf"):
        t = float(name[5:])
        want = {"accepted": 1}
        if t == 0.5 and M == 5:  # a handful of particles within half a pixel: no early exit, still accepted
            want.update(iters=80, few_weights=True)
        return mk(prm={"tol_pf": t}, pk_ok=True, want=want)
    raise KeyError(name)


PRED_NAMES = ["base", "ang0.0255", "ang0.0256", "ang0.3-force25", "ang1.0-it1", "ang1.0-it2", "neg-growth", "cam",
              "K2", "Krot", "Kskew", "nan0", "inf0", "nan7", "fewer-blobs", "tolpf0.5", "tolpf7", "tolpf30"]
PRED_FP16_NAMES = ["base", "ang0.0255", "ang0.0256", "cam", "K2", "Krot", "Kskew"]
PRED_CASES = [(b, n) for b in BASELINES for n in PRED_NAMES]
PRED_FP16_CASES = [(b, n) for b in BASELINES for n in PRED_FP16_NAMES]


def pred_id(case):
    return f"{case[0]}-{case[1]}"


@functools.lru_cache(maxsize=None)
def pred_case(base, name):
    return [_predicate(base, name)]


def all_fp32_frames():
    """Every frame that runs in fp32 or fp16 state (each needs its distance from the tol_PF gate checked)."""
    out = []
    for c in MARKER_CASES:
        out += marker_case(*c)
    for M in EXTRA_MS:
        out += marker_extra(M)
    for c in BLOB_CASES:
        out += blob_case(*c)
    for c in PRED_CASES:
        out += pred_case(*c)
    return out
