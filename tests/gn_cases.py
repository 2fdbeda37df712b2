"""The case list of the Gauss-Newton envelope (tests/test_gn_envelope_host.py, tests/test_gpu_gn_envelope.py).

refine_ref.py's three clouds meet the refinement in one corner: one scene time, three models, K_README, the default
parameters, hypotheses near the truth.  A case here is a model, K, a blob list, up to 700 start poses (two full
256-lane blocks and a partial one), their pair rows and the refinement parameters:

  buckets     M in MARKER_MS, B = max(M, 20) light and, from M = 6, 200 heavy; truth_pose(3.0), initial_prior(T, 700),
              the pairs of the oracle's likelihood
  scenes      truth_pose(0.5) and truth_pose(1.7) at M = 4, 5, 12: where Gauss-Newton crawls (half the rows of 0.5 stop
              at the cap) and where it takes 14-17 iterations
  far starts  M = 5 and 12, every LED paired with its exact projection, the start pose T exp([0; a axis]) for
              a in FAR_ANGLES and 64 random axes each: first steps of several radians, which take gn_sincos through
              all four quarter-turn cases, and rows that stop at the cap, kept and reverted
  parameters  max_iter in {1, 2, 3, 10000}, converged in {0, 1e-6}, the divergence rule on and off, on the 0.5 scene
  K           2 K, a skew term, K Rx(0.01) Ry(-0.02) with the blobs mapped through the same homography; M = 5
  degenerate  one list of rows that are singular, non-finite or oddly paired (degenerate_case)
  ties        one hypothesis repeated in different lanes of a wave, in different waves and in different blocks

The oracle's optimisePose has the default parameters built in, so only cases with `oracle` set are compared with it;
the others are compared host against device, and the host against what the iteration does not touch.
Everything here is computed once per session and shared; do not modify what the functions return.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

import refine_ref as rr
from test_gpu_refine import best_of  # numpy's argbest of a call's rows (no GPU involved)

N = 700
MARKER_MS = [1, 2, 3, 4, 6, 8, 9, 11, 13, 16]
SCENE_TIMES = [0.5, 1.7]
SCENE_MS = [4, 5, 12]
FAR_ANGLES = [1.6, 2.4, 3.1]
FAR_AXES = 64
TIE_AT = [37, 41, 100, 300, 650]  # lanes 37 and 41 of wave 0, wave 1 of block 0, blocks 1 and 2


@dataclass
class Case:
    name: str
    markers: np.ndarray
    K: np.ndarray
    blobs: np.ndarray
    poses: np.ndarray  # (n, 12)
    pairs: np.ndarray  # (n, MAX_MARKERS, 2) uint32
    prm: dict = field(default_factory=dict)  # fields of pf.RefineParams away from their defaults
    oracle: bool = True  # default parameters: the oracle's optimisePose applies
    group: str = ""
    note: dict = field(default_factory=dict)  # what the builder knows about its rows (indices by kind)


def params(case: Case):
    p = pf.default_refine_params()
    for k, v in case.prm.items():
        setattr(p, k, v)
    return p


def _freeze(c: Case) -> Case:
    for a in (c.markers, c.K, c.blobs, c.poses, c.pairs):
        a.setflags(write=False)
    return c


def _scene_case(name, M, heavy, t, group, blob_seed=0, K=None, n=N, B=None) -> Case:
    """One frame of the synthetic stream at truth_pose(t) and the cloud initial_prior(T, n) around it."""
    B = B or (200 if heavy else max(M, 20))
    cfg = syn.StreamConfig(name, M=M, B=B, N=0, heavy=heavy, seed=blob_seed)
    markers = syn.markers_for(M)
    T = syn.truth_pose(t)
    blobs = syn.blobs_for_frame(cfg, T, 0, markers)
    K0 = syn.K_README.copy()
    if K is not None:  # the frame seen through K: the blobs mapped by the homography K K0^-1, like the projections
        h = (K @ np.linalg.inv(K0) @ np.column_stack([blobs, np.ones(len(blobs))]).T).T
        blobs = (h[:, :2] / h[:, 2:3]).astype(np.float32).astype(np.float64)
        K0 = np.array(K, dtype=np.float64)
    poses = syn.initial_prior(T, n)
    pairs = rr.oracle_pairs(markers, K0, blobs, poses)
    return Case(name, markers, K0, blobs, poses, pairs, group=group)


# ------------------------------------------------------------------------------------------------- buckets
BUCKET_CASES = [(M, False) for M in MARKER_MS] + [(M, True) for M in MARKER_MS if M >= 6]


def bucket_id(c):
    return f"M{c[0]}-{'heavy' if c[1] else 'light'}"


@functools.lru_cache(maxsize=None)
def bucket_case(M, heavy) -> Case:
    return _freeze(_scene_case(bucket_id((M, heavy)), M, heavy, rr.SCENE_T, "bucket"))


# -------------------------------------------------------------------------------------------------- scenes
SCENE_CASES = [(t, M) for t in SCENE_TIMES for M in SCENE_MS]


def scene_id(c):
    return f"t{c[0]}-M{c[1]}"


@functools.lru_cache(maxsize=None)
def scene_case(t, M) -> Case:
    return _freeze(_scene_case(scene_id((t, M)), M, M == 12, t, f"scene{t}", B=40 if M == 12 else None))


# ---------------------------------------------------------------------------------------------- far starts
FAR_MS = [5, 12]


@functools.lru_cache(maxsize=None)
def far_case(M) -> Case:
    markers = syn.markers_for(M)
    K = syn.K_README.copy()
    T = syn.truth_pose(rr.SCENE_T)
    blobs = syn.project(K, T, markers)
    rng = np.random.default_rng(300 + M)
    poses, angle = [], []
    for a in FAR_ANGLES:
        for _ in range(FAR_AXES):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            poses.append(syn.to12(T @ syn.se3_exp(np.concatenate([np.zeros(3), a * axis]))))
            angle.append(a)
    pairs = np.zeros((len(poses), pf.MAX_MARKERS, 2), dtype=np.uint32)
    pairs[:, :M, 0] = pairs[:, :M, 1] = np.arange(1, M + 1, dtype=np.uint32)
    return _freeze(Case(f"far-M{M}", markers, K, blobs, np.array(poses), pairs, group="far",
                        note={"angle": np.array(angle)}))


def first_step(case: Case, i: int) -> np.ndarray:
    """The first Gauss-Newton step of hypothesis i, [upsilon; omega], from numpy's own solve of the normal equations
    (computeJacobian, PE:2163-2192)."""
    P = case.poses[i].reshape(3, 4)
    fx, fy = case.K[0, 0], case.K[1, 1]
    A, b = np.zeros((6, 6)), np.zeros(6)
    for led, blob in case.pairs[i]:
        if blob == 0:
            continue
        X = case.markers[led - 1]
        x, y, z = P[:, :3] @ X + P[:, 3]
        p = case.K @ np.array([x, y, z])
        e = case.blobs[blob - 1] - p[:2] / p[2]
        J = np.array([[fx / z, 0, -x / z ** 2 * fx, -x * y / z ** 2 * fx, (1 + x * x / z ** 2) * fx, -y / z * fx],
                      [0, fy / z, -y / z ** 2 * fy, -(1 + y * y / z ** 2) * fy, x * y / z ** 2 * fy, x / z * fy]])
        A += J.T @ J
        b += J.T @ e
    return np.linalg.solve(A, b)


# ---------------------------------------------------------------------------------------------- parameters
PARAM_SETS = {
    "it1": {"max_iter": 1}, "it2": {"max_iter": 2}, "it3": {"max_iter": 3}, "it10000": {"max_iter": 10000},
    "conv0": {"converged": 0.0}, "conv1e-6": {"converged": 1e-6},
    "it3-conv1e-6": {"max_iter": 3, "converged": 1e-6}, "it10000-conv0": {"max_iter": 10000, "converged": 0.0},
    "it3-keep": {"max_iter": 3, "revert_on_divergence": 0}, "keep": {"revert_on_divergence": 0},
}
PARAM_ROWS = {"it10000": 128, "it10000-conv0": 64}  # rows with pairs: the long runs on fewer (every other set: 192)
PARAM_CASES = [(M, name) for M in (4, 5) for name in PARAM_SETS]


def param_id(c):
    return f"M{c[0]}-{c[1]}"


@functools.lru_cache(maxsize=None)
def param_case(M, name) -> Case:
    base = scene_case(0.5, M)
    paired = np.count_nonzero(base.pairs[:, :, 1], axis=1) > 0
    sel = np.sort(np.concatenate([np.flatnonzero(paired)[: PARAM_ROWS.get(name, 192)], np.flatnonzero(~paired)[:8]]))
    return _freeze(Case(f"param-{param_id((M, name))}", base.markers, base.K, base.blobs, base.poses[sel].copy(),
                        base.pairs[sel].copy(), prm=dict(PARAM_SETS[name]), oracle=False, group="param",
                        note={"sel": sel}))  # sel: the rows of scene_case(0.5, M)


# ------------------------------------------------------------------------------------------------------- K
K_NAMES = ["K2", "Kskew", "Krot"]


@functools.lru_cache(maxsize=None)
def k_case(name) -> Case:
    K = syn.K_README.copy()
    if name == "K2":
        K = 2.0 * K
    elif name == "Kskew":
        K[0, 1] = 0.7
    elif name == "Krot":
        K = K @ syn.rot_x(0.01) @ syn.rot_y(-0.02)
    else:
        raise KeyError(name)
    return _freeze(_scene_case(name, 5, False, rr.SCENE_T, "K", K=K))


# ---------------------------------------------------------------------------------------------- degenerate
@functools.lru_cache(maxsize=None)
def degenerate_case() -> Case:
    """A 16-LED model whose LED 1 sits at the model origin.  Blobs 1..16: the LEDs' exact projections at
    truth_pose(3.0); 17: the principal point (the on-axis LED's projection); 18: 3 px beside it; 19: NaN x;
    20: +inf y.  note[kind] lists the rows of each kind."""
    M = 16
    markers = syn.markers_for(M)
    markers[0] = 0.0
    K = syn.K_README.copy()
    T = syn.truth_pose(rr.SCENE_T)
    blobs = np.vstack([syn.project(K, T, markers), [K[0, 2], K[1, 2]], [K[0, 2] + 3.0, K[1, 2] - 1.0],
                       [np.nan, 100.0], [100.0, np.inf]])
    near = syn.initial_prior(T, 64, seed=11)
    axis_pose = lambda z: np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, z])
    full = [(l, l) for l in range(1, M + 1)]
    rows, note = [], {}

    def add(kind, pose, pr):
        pad = np.zeros((pf.MAX_MARKERS, 2), dtype=np.uint32)
        pad[: len(pr)] = pr
        note.setdefault(kind, []).append(len(rows))
        rows.append((np.array(pose, dtype=np.float64), pad))

    k = 0
    for z in (2.0, 0.75, 3.5):  # one pair, its LED on the optical axis: A[2][2] and A[5][5] are exactly 0
        add("on_axis", axis_pose(z), [(1, 17)])
    add("on_axis", axis_pose(2.0), [(1, 18)])  # the same with a residual: the zero pivot decides, not b = 0
    for t in ((0.1, 0.1, 0.0), (-0.2, 0.05, 0.0)):  # the paired LED in the camera's plane z = 0
        p = axis_pose(0.0)
        p[[3, 7]] = t[:2]
        add("z0", p, [(1, 1)])
        add("z0", p, full)
    for i in range(3):  # the object behind the camera
        p = near[k + i].copy()
        p[11] = -p[11]
        add("behind", p, full[:5 + i])
    k += 3
    for i in range(3):
        add("nan_x", near[k + i], full[:2] + [(3, 19)] + full[3:6 + i])
        add("inf_y", near[k + i], full[:4] + [(5, 20)] + full[5:7 + i])
    k += 3
    for i in range(3):
        add("two_leds_one_blob", near[k + i], full[:6 + i] + [(3, 2)])
        add("led_twice", near[k + i], full[:6 + i] + [(2, 2)])
        add("led_twice", near[k + i], full[:6 + i] + [(2, 3)])
    k += 3
    for i in range(6):
        add("all16", near[k + i], full)
    k += 6
    for i in range(3):
        add("holes", near[k + i], [(1, 1), (2, 0), (3, 3), (0, 0), (5, 5), (6, 6), (7, 0), (8, 8), (0, 0), (10, 10)][: 7 + i])
    k += 3
    for i in range(3):
        add("no_pairs", near[k + i], np.zeros((0, 2), dtype=np.uint32) if i == 0 else [(1, 0), (4, 0), (0, 0)])
    poses = np.array([r[0] for r in rows])
    pairs = np.array([r[1] for r in rows])
    return _freeze(Case("degenerate", markers, K, blobs, poses, pairs, group="degenerate",
                        note={k_: np.array(v) for k_, v in note.items()}))


# ---------------------------------------------------------------------------------------------------- ties
@functools.lru_cache(maxsize=None)
def tie_case() -> Case:
    """M5-light's rows with its best hypothesis (by the host's rows) copied to TIE_AT: equal best keys in two lanes of
    a wave, in two waves of a block and in three blocks.  The lowest index must win; note["best"] is that index."""
    base = bucket_case_5()
    rows, _ = host_rows(base)
    b = best_of(rows)
    poses, pairs = base.poses.copy(), base.pairs.copy()
    for i in TIE_AT:
        poses[i], pairs[i] = base.poses[b], base.pairs[b]
    return _freeze(Case("ties", base.markers, base.K, base.blobs, poses, pairs, group="ties",
                        note={"best": min(TIE_AT + [b]), "copies": sorted(set(TIE_AT + [b]))}))


@functools.lru_cache(maxsize=None)
def bucket_case_5() -> Case:
    """The 5-LED model (the exact-5 bucket is not in MARKER_MS: refine_ref's cloud A covers it) as a bucket case."""
    return _freeze(_scene_case("M5-light", 5, False, rr.SCENE_T, "bucket"))


# ------------------------------------------------------------------------------------------------ the list
def all_cases() -> list:
    out = [bucket_case(*c) for c in BUCKET_CASES]
    out += [scene_case(*c) for c in SCENE_CASES]
    out += [far_case(M) for M in FAR_MS]
    out += [param_case(*c) for c in PARAM_CASES]
    out += [k_case(n) for n in K_NAMES]
    out += [degenerate_case(), tie_case()]
    return out


CASE_IDS = ([bucket_id(c) for c in BUCKET_CASES] + [scene_id(c) for c in SCENE_CASES] + [f"far-M{M}" for M in FAR_MS] +
            [f"param-{param_id(c)}" for c in PARAM_CASES] + K_NAMES + ["degenerate", "ties"])


def case_by_id(cid) -> Case:
    i = CASE_IDS.index(cid)
    nb, ns, nf, npar = len(BUCKET_CASES), len(SCENE_CASES), len(FAR_MS), len(PARAM_CASES)
    if i < nb:
        return bucket_case(*BUCKET_CASES[i])
    i -= nb
    if i < ns:
        return scene_case(*SCENE_CASES[i])
    i -= ns
    if i < nf:
        return far_case(FAR_MS[i])
    i -= nf
    if i < npar:
        return param_case(*PARAM_CASES[i])
    i -= npar
    if i < len(K_NAMES):
        return k_case(K_NAMES[i])
    return degenerate_case() if cid == "degenerate" else tie_case()


# ----------------------------------------------------------------------------------- the host's rows, shared
_HOST = {}


def host_rows(case: Case):
    """pfmpe_host_optimise_pose over the case: (rows, cov), once per session.  Do not modify."""
    hit = _HOST.get(case.name)
    if hit is None:
        n = len(case.poses)
        rows = np.zeros(n, dtype=pf.REFINE_ROW_DTYPE)
        cov = np.zeros((n, 6, 6))
        p = params(case)
        for i in range(n):
            rows[i], cov[i] = pf.host_optimise_pose(case.markers, case.K, case.blobs, case.pairs[i], case.poses[i], p)
        rows.setflags(write=False)
        cov.setflags(write=False)
        hit = _HOST[case.name] = (rows, cov)
    return hit

