"""pfmpe_host_cloud_assign, the assignment of pfmpe_cloud_modes on the host, against a numpy restatement written with
the same operand order (tests/cloud_modes_ref.py), its edge cases and error codes, and the layout of the call's two
structs.  No GPU.

Every comparison is exact.  That needs inputs on which no decision sits on a rounding: each case asserts, for every
particle and with the numpy numbers alone, that its two smallest distances differ by more than a relative 1e-9 (and
that its smallest distance is not within 1e-9 of the gate)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

import cloud_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [1, 2, 3, 16])
@pytest.mark.parametrize("N", [0, 1, 257, 300_001])
def test_assign_equals_numpy(N, K):
    seeds = ref.seeds(K)
    for gen_seed in (1, 2, 3):
        for through_fp32 in (False, True):
            P = ref.cloud(300_001, gen_seed, through_fp32)[:N]
            gap = ref.assert_margin(P, seeds)
            want_mode, want_counts, _ = ref.assign(P, seeds)
            mode_of, counts = pf.host_cloud_assign(P, seeds)
            assert np.array_equal(mode_of, want_mode), (gen_seed, through_fp32)
            assert np.array_equal(counts, want_counts) and counts.sum() == N and counts[K] == 0
            if N == 300_001 and K == 3:
                print(f"seed {gen_seed} fp32 {through_fp32}: smallest relative gap {gap:.3e}, counts {counts}")
                own = np.random.default_rng(gen_seed).integers(0, 3, N)  # the draw cloud() begins with
                crossed = np.mean(mode_of != own)
                assert 0.005 < crossed < 0.05, crossed  # the boundary between the modes is exercised


@pytest.mark.parametrize("max_dist", [1.0, 4.0, 20.0])
def test_gate_equals_numpy(max_dist):
    N, seeds = 100_003, ref.seeds(3)
    P = ref.cloud(300_001, 2, True)[:N]
    ref.assert_margin(P, seeds, max_dist=max_dist)
    want_mode, want_counts, _ = ref.assign(P, seeds, max_dist=max_dist)
    mode_of, counts = pf.host_cloud_assign(P, seeds, max_dist=max_dist)
    assert np.array_equal(mode_of, want_mode) and np.array_equal(counts, want_counts)
    assert counts.sum() == N and 0 < counts[3] < N  # the gate leaves some out and some in


def _pose(t=(0.0, 0.0, 1.0), w=(0.0, 0.0, 0.0)):
    return ref.rows(ref.rodrigues(np.array([w])), np.array([t], dtype=np.float64))[0]


def test_ties_go_to_the_lower_index():
    P = ref.cloud(4097, 1)
    s = ref.seeds(3)
    seeds = np.stack([s[1], s[0], s[1], s[0]])  # seeds 2 and 3 repeat 0 and 1 bit for bit
    mode_of, counts = pf.host_cloud_assign(P, seeds)
    assert set(np.unique(mode_of)) == {0, 1} and counts[2] == 0 and counts[3] == 0 and counts[4] == 0
    want, _ = pf.host_cloud_assign(P, seeds[:2])
    assert np.array_equal(mode_of, want)
    both, counts = pf.host_cloud_assign(P, np.stack([s[0], s[0]]))
    assert np.all(both == 0) and list(counts) == [4097, 0, 0]


def test_gate_by_hand():
    """Translation only, scale 0.01 m: a particle d metres from the seed has dist = (d / 0.01)^2.  max_dist = 4 is a
    radius of 2 cm; particles at 1.9 and 2.1 cm, and one exactly on the gate (d2 * it2 == 4 needs no rounding at
    d = 2^-6 m with scale 2^-7 m), which is inside (best <= max_dist)."""
    seed = _pose()
    P = np.stack([_pose((0.019, 0, 1)), _pose((0.021, 0, 1)), _pose((0, -0.019, 1)), _pose((0, 0, 1.021)), seed])
    mode_of, counts = pf.host_cloud_assign(P, seed, trans_scale=0.01, rot_scale=0.0, max_dist=4.0)
    assert list(mode_of) == [0, pf.MODE_NONE, 0, pf.MODE_NONE, 0] and list(counts) == [3, 2]
    mode_of, counts = pf.host_cloud_assign(P, seed, trans_scale=0.01, rot_scale=0.0, max_dist=0.0)
    assert list(mode_of) == [0] * 5 and list(counts) == [5, 0]  # no gate
    on = np.stack([_pose((2.0 ** -6, 0, 1)), _pose((np.nextafter(2.0 ** -6, 1), 0, 1))])
    mode_of, _ = pf.host_cloud_assign(on, seed, trans_scale=2.0 ** -7, rot_scale=0.0, max_dist=4.0)
    assert list(mode_of) == [0, pf.MODE_NONE]
    # rotation only: 3 - tr = 2 (1 - cos theta), so theta = 0.1 rad at scale 0.05 rad is dist ~ 3.997
    rot = np.stack([_pose(w=(0.1, 0, 0)), _pose(w=(0, 0.101, 0)), _pose((5.0, 5.0, 5.0), w=(0, 0, 0.05))])
    mode_of, _ = pf.host_cloud_assign(rot, seed, trans_scale=0.0, rot_scale=0.05, max_dist=4.0)
    assert list(mode_of) == [0, pf.MODE_NONE, 0]  # (the translation does not count)


def test_non_finite_poses_have_no_mode():
    seeds = ref.seeds(3)
    P = ref.cloud(64, 1).copy()
    P[3, 7] = np.nan      # a NaN translation
    P[10, 5] = np.nan     # a NaN rotation entry
    P[20, 11] = np.inf    # an infinite translation: dist = +inf
    P[30, 0] = np.inf     # infinite rotation entries: tr = +-inf or NaN, dist = -+inf or NaN
    P[31, 0] = -np.inf
    P[40, :] = np.inf
    bad = [3, 10, 20, 30, 31, 40]
    for max_dist in (0.0, 50.0):
        mode_of, counts = pf.host_cloud_assign(P, seeds, max_dist=max_dist)
        assert np.all(mode_of[bad] == pf.MODE_NONE)
        good = np.setdiff1d(np.arange(64), bad)
        want, _, _ = ref.assign(P[good], seeds, max_dist=max_dist)
        assert np.array_equal(mode_of[good], want)
        assert counts.sum() == 64 and counts[3] >= len(bad)
    want, _, _ = ref.assign(P, seeds)
    assert np.array_equal(pf.host_cloud_assign(P, seeds)[0], want)  # the restatement has the same rule


def test_one_scale_zero():
    P, seeds = ref.cloud(4097, 3), ref.seeds(3)
    for ts, rs in ((0.01, 0.0), (0.0, 0.05)):
        ref.assert_margin(P, seeds, ts, rs)
        want_mode, want_counts, _ = ref.assign(P, seeds, ts, rs)
        mode_of, counts = pf.host_cloud_assign(P, seeds, trans_scale=ts, rot_scale=rs)
        assert np.array_equal(mode_of, want_mode) and np.array_equal(counts, want_counts)
    # translation does not count: seeds that differ in translation alone tie, and the lower index takes everything
    far = seeds[0].copy()
    far[[3, 7, 11]] += 1.0
    mode_of, _ = pf.host_cloud_assign(P, np.stack([far, seeds[0]]), trans_scale=0.0, rot_scale=0.05)
    assert np.all(mode_of == 0)


def _raw(poses, N, seeds, K, prm, null=()):
    """The C call with sentinels in both outputs; returns (code, outputs untouched)."""
    lib = pf.load()
    mode_of = np.full(16, 0x5A, dtype=np.uint8)
    counts = np.full(pf.MODES_MAX + 1, -77, dtype=np.int64)
    dp = C.POINTER(C.c_double)
    p = None if prm is None else _capi.ModesParams(*prm)
    rc = lib.pfmpe_host_cloud_assign(
        None if "poses" in null else poses.ctypes.data_as(dp), N,
        None if "seeds" in null else seeds.ctypes.data_as(dp), K, None if p is None else C.byref(p),
        None if "mode_of" in null else mode_of.ctypes.data_as(C.POINTER(C.c_uint8)),
        None if "counts" in null else counts.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, bool(np.all(mode_of == 0x5A) and np.all(counts == -77)), mode_of, counts


def test_error_codes_leave_outputs_untouched():
    P = np.ascontiguousarray(ref.cloud(4, 1))
    seeds = np.ascontiguousarray(ref.seeds(16))
    many = np.ascontiguousarray(np.vstack([seeds, seeds[:1]]))
    nan_seed, inf_seed = seeds.copy(), seeds.copy()
    nan_seed[1, 4] = np.nan
    inf_seed[0, 3] = np.inf
    nan, inf = float("nan"), float("inf")
    ok = (0.01, 0.05, 0.0)
    bad = [
        (P, 4, seeds, 2, ok, ("poses",)), (P, 4, seeds, 2, ok, ("seeds",)), (P, 4, seeds, 2, ok, ("mode_of",)),
        (P, -1, seeds, 2, ok, ()), (P, 4, seeds, 0, ok, ()), (P, 4, seeds, -1, ok, ()),
        (P, 4, many, pf.MODES_MAX + 1, ok, ()), (P, 4, nan_seed, 2, ok, ()), (P, 4, inf_seed, 2, ok, ()),
        (P, 4, seeds, 2, (-0.01, 0.05, 0.0), ()), (P, 4, seeds, 2, (nan, 0.05, 0.0), ()),
        (P, 4, seeds, 2, (inf, 0.05, 0.0), ()), (P, 4, seeds, 2, (0.01, -0.05, 0.0), ()),
        (P, 4, seeds, 2, (0.01, nan, 0.0), ()), (P, 4, seeds, 2, (0.01, inf, 0.0), ()),
        (P, 4, seeds, 2, (0.01, 0.05, -1.0), ()), (P, 4, seeds, 2, (0.01, 0.05, nan), ()),
        (P, 4, seeds, 2, (0.01, 0.05, inf), ()), (P, 4, seeds, 2, (0.0, 0.0, 0.0), ()),
    ]
    for args in bad:
        rc, untouched, _, _ = _raw(*args)
        assert rc == pf.E_ARG, args[1:]
        assert untouched, args[1:]
    # the non-finite seed lies behind the K seeds in use: not read
    assert _raw(P, 4, nan_seed, 1, ok)[0] == pf.OK
    # the edges of the valid ranges; NULL params are the defaults; NULL counts, and NULL poses / mode_of with N = 0
    for args in [(P, 4, seeds, 1, ok, ()), (P, 4, seeds, pf.MODES_MAX, ok, ()), (P, 4, seeds, 2, (0.0, 0.05, 0.0), ()),
                 (P, 4, seeds, 2, (0.01, 0.0, 3.0), ()), (P, 4, seeds, 2, None, ()), (P, 4, seeds, 2, ok, ("counts",)),
                 (P, 0, seeds, 2, ok, ("poses", "mode_of"))]:
        rc, _, mode_of, counts = _raw(*args)
        assert rc == pf.OK, args[1:]
        if "counts" not in args[5]:
            assert counts[: args[3] + 1].sum() == args[1] and np.all(counts[args[3] + 1:] == -77)
        assert np.all(mode_of[args[1]:] == 0x5A)
    a = _raw(P, 4, seeds, 3, None)
    b = _raw(P, 4, seeds, 3, ok)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_struct_sizes_and_defaults():
    assert C.sizeof(_capi.ModesParams) == 24
    assert C.sizeof(_capi.ModeOut) == 488 and C.sizeof(_capi.CloudOut) == 480
    assert _capi.ModeOut.share.offset == 480
    p = pf.default_modes_params()
    assert (p.trans_scale, p.rot_scale, p.max_dist) == (0.01, 0.05, 0.0)


def test_constants_and_symbols_match_header():
    hdr = open(os.path.join(ROOT, "include", "pfmpe.h")).read()
    assert int(re.search(r"#define PFMPE_MODES_MAX\s+(\d+)", hdr).group(1)) == pf.MODES_MAX
    assert int(re.search(r"#define PFMPE_MODE_NONE\s+(\d+)", hdr).group(1)) == pf.MODE_NONE == ref.MODE_NONE
    lib = pf.load()
    for name in ("pfmpe_default_modes_params", "pfmpe_cloud_modes", "pfmpe_host_cloud_assign"):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr)
