"""pfmpe_host_top_suppress, the suppression walk of pfmpe_top_particles on the host, against a numpy restatement of
the walk (numpy rounds every product and sum on its own, as the predicate is defined), its error codes, and the
layout of the call's two structs.  No GPU.

Every comparison is exact.  That needs inputs on which no decision sits on a rounding: each case asserts that no
pair's d2 or tr lies within a relative 1e-9 of its threshold (a condition on the inputs, checked with the numpy
numbers alone)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
T_IDX = [3, 7, 11]
R_IDX = [0, 1, 2, 4, 5, 6, 8, 9, 10]


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def random_poses(P, seed, trans_sigma=0.005, rot_sigma=0.05):
    """P poses scattered about one pose: a few mm and a few hundredths of a radian apart, so that thresholds of that
    size keep some and drop some.  (tr lies near 3 whatever the angle, so a relative margin on it is a wide window in
    the angle: the rotations are spread widely enough that no pair of these seeds falls into it.)"""
    rng = np.random.default_rng(seed)
    base_R = rodrigues(np.array([0.3, -0.2, 0.5]))
    base_t = np.array([0.1, -0.05, 1.5])
    out = np.zeros((P, 12))
    for n in range(P):
        R = rodrigues(rng.normal(0, rot_sigma, 3)) @ base_R
        t = base_t + rng.normal(0, trans_sigma, 3)
        out[n] = np.hstack([R, t[:, None]]).reshape(-1)
    return out


def pair_terms(pj, pi):
    """d2 and tr of pose(s) pj against pose(s) pi, in the order the definition writes them."""
    d = pj[..., T_IDX] - pi[..., T_IDX]
    d2 = d[..., 0] * d[..., 0]
    d2 = d2 + d[..., 1] * d[..., 1]
    d2 = d2 + d[..., 2] * d[..., 2]
    a, b = pj[..., R_IDX], pi[..., R_IDX]
    tr = a[..., 0] * b[..., 0]
    for k in range(1, 9):
        tr = tr + a[..., k] * b[..., k]
    return d2, tr


def thresholds(min_trans, min_rot):
    return min_trans * min_trans, 1.0 + 2.0 * math.cos(min_rot)


def assert_margin(poses, min_trans, min_rot):
    """No pair of the list decides within MARGIN of a threshold (all pairs: a superset of those the walk meets)."""
    P = len(poses)
    if P < 2:
        return
    t2, rc = thresholds(min_trans, min_rot)
    for j0 in range(0, P, 256):  # in slabs: P x P x 9 doubles at once is more than this needs
        d2, tr = pair_terms(poses[j0:j0 + 256, None, :], poses[None, :, :])
        if min_trans != 0:
            assert np.all(np.abs(d2 - t2) > MARGIN * t2), "an input pair sits on the translation threshold"
        if min_rot != 0:
            assert np.all(np.abs(tr - rc) > MARGIN * abs(rc)), "an input pair sits on the rotation threshold"


def numpy_walk(poses, K, min_trans, min_rot):
    t2, rc = thresholds(min_trans, min_rot)
    suppress = min_trans != 0 or min_rot != 0
    keep = []
    j = 0
    P = len(poses)
    while j < P and len(keep) < K:
        near = False
        if suppress and keep:
            d2, tr = pair_terms(poses[j][None, :], poses[keep])
            near_t = np.ones(len(keep), dtype=bool) if min_trans == 0 else d2 < t2
            near_r = np.ones(len(keep), dtype=bool) if min_rot == 0 else tr > rc
            near = bool(np.any(near_t & near_r))
        if not near:
            keep.append(j)
        j += 1
    return np.array(keep, dtype=np.int32), j


CASES = {
    "translation": (0.004, 0.0),
    "rotation": (0.0, 0.03),
    "both": (0.006, 0.06),
    "none": (0.0, 0.0),
    "huge": (10.0, math.pi),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("K", [0, 1, 8, 1024])
@pytest.mark.parametrize("P", [0, 1, 2, 65, 1024, 1500])
def test_walk_equals_numpy(P, K, case):
    min_trans, min_rot = CASES[case]
    poses = random_poses(P, seed=1000 + P)
    assert_margin(poses, min_trans, min_rot)
    want_keep, want_ex = numpy_walk(poses, K, min_trans, min_rot)
    got = pf.host_top_suppress(poses, K, min_trans, min_rot)
    assert got["n_out"] == len(want_keep) and got["n_examined"] == want_ex
    assert np.array_equal(got["keep"], want_keep)
    if case == "none":
        assert got["n_out"] == min(K, P) and got["n_examined"] == got["n_out"]
        assert np.array_equal(got["keep"], np.arange(min(K, P)))
    if case == "huge" and K >= 2 and P >= 1:  # everything is near the first: one kept, the whole list walked
        assert got["n_out"] == 1 and got["n_examined"] == P
    if case in ("translation", "rotation", "both") and P >= 1024 and K == 1024:
        assert 1 < got["n_out"] < P  # the thresholds do separate: some kept, some dropped


@pytest.mark.parametrize("min_trans,min_rot", [(1e-6, 0.0), (0.0, 1e-4), (1e-6, 1e-4), (0.004, 0.03)])
def test_bit_equal_poses(min_trans, min_rot):
    """The second of two bit-equal poses is suppressed by any positive threshold."""
    poses = random_poses(6, seed=7, trans_sigma=0.05, rot_sigma=0.3)
    poses[3] = poses[1]
    assert_margin(poses, min_trans, min_rot)
    got = pf.host_top_suppress(poses, 8, min_trans, min_rot)
    want_keep, want_ex = numpy_walk(poses, 8, min_trans, min_rot)
    assert np.array_equal(got["keep"], want_keep) and got["n_examined"] == want_ex
    assert 1 in got["keep"] and 3 not in got["keep"]


def _raw(poses, P, K, min_trans, min_rot, null=()):
    """The C call with sentinels in every output; returns (code, outputs untouched)."""
    lib = pf.load()
    keep = np.full(1024, -77, dtype=np.int32)
    n_out, n_ex = C.c_int32(-5), C.c_int32(-6)
    ip = C.POINTER(C.c_int32)
    rc = lib.pfmpe_host_top_suppress(
        None if "poses" in null else poses.ctypes.data_as(C.POINTER(C.c_double)), P, K, min_trans, min_rot,
        None if "keep" in null else keep.ctypes.data_as(ip), None if "n_out" in null else C.byref(n_out),
        None if "n_examined" in null else C.byref(n_ex))
    return rc, bool(np.all(keep == -77) and n_out.value == -5 and n_ex.value == -6)


def test_error_codes_leave_outputs_untouched():
    poses = random_poses(4, seed=3)
    bad_nan, bad_inf = poses.copy(), poses.copy()
    bad_nan[2, 5] = np.nan
    bad_inf[3, 11] = np.inf
    nan, inf = float("nan"), float("inf")
    bad = [
        (poses, 4, 2, 0.01, 0.1, ("poses",)), (poses, 4, 2, 0.01, 0.1, ("keep",)), (poses, 4, 2, 0.01, 0.1, ("n_out",)),
        (poses, 4, 2, 0.01, 0.1, ("n_examined",)),
        (poses, -1, 2, 0.01, 0.1, ()), (poses, 4, -1, 0.01, 0.1, ()), (poses, 4, pf.TOP_MAX + 1, 0.01, 0.1, ()),
        (poses, 4, 2, -0.01, 0.1, ()), (poses, 4, 2, inf, 0.1, ()), (poses, 4, 2, nan, 0.1, ()),
        (poses, 4, 2, 0.01, -0.1, ()), (poses, 4, 2, 0.01, math.pi + 1e-9, ()), (poses, 4, 2, 0.01, nan, ()),
        (bad_nan, 4, 2, 0.01, 0.1, ()), (bad_inf, 4, 2, 0.0, 0.0, ()),
    ]
    for args in bad:
        rc, untouched = _raw(*args)
        assert rc == pf.E_ARG, args[1:]
        assert untouched, args[1:]
    # the edges of the valid ranges are accepted
    for args in [(poses, 4, 0, 0.0, 0.0, ()), (poses, 4, pf.TOP_MAX, 0.0, math.pi, ()), (poses, 0, 8, 0.01, 0.1, ())]:
        rc, _ = _raw(*args)
        assert rc == pf.OK, args[1:]


def test_struct_sizes_and_defaults():
    assert C.sizeof(_capi.TopParams) == 24
    assert C.sizeof(_capi.TopOut) == 24
    p = pf.default_top_params()
    assert (p.key, p.K, p.min_trans, p.min_rot) == (pf.TOP_BY_WEIGHT, 8, 0.0, 0.0)


def test_constants_match_header():
    hdr = open(os.path.join(ROOT, "include", "pfmpe.h")).read()
    assert int(re.search(r"#define PFMPE_TOP_MAX\s+(\d+)", hdr).group(1)) == pf.TOP_MAX
    assert int(re.search(r"#define PFMPE_TOP_POOL\s+(\d+)", hdr).group(1)) == pf.TOP_POOL
    m = re.search(r"enum \{ PFMPE_TOP_BY_WEIGHT = (\d+), PFMPE_TOP_BY_COUNT = (\d+) \}", hdr)
    assert (int(m.group(1)), int(m.group(2))) == (pf.TOP_BY_WEIGHT, pf.TOP_BY_COUNT)
