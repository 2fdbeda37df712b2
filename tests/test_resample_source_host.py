"""The index rule of pfmpe_resample_prior on the host (pfmpe_host_resample_source, pfmpe_host_resample_rank): the rank
r = ((2k + 1) m) / (2 n_new) against a Python big-integer restatement, the properties include/pfmpe.h states for it,
the members of a mode assigned by pfmpe_host_cloud_assign, and the argument errors.  Integers only: every check is
exact."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf

import cloud_modes_ref as ref

SIZES = [1, 2, 255, 256, 257, 4097]
BIG = 2**31 - 1


def rank(k, m, n_new):
    return ((2 * int(k) + 1) * int(m)) // (2 * int(n_new))


@pytest.mark.parametrize("n_new", SIZES)
@pytest.mark.parametrize("m", SIZES)
def test_rank_rule_and_its_properties(m, n_new):
    source, members = pf.host_resample_source(None, 0, n_new, N=m)  # every particle a member: source[k] is the rank
    assert members == m and source.dtype == np.int32 and len(source) == n_new
    assert source.tolist() == [rank(k, m, n_new) for k in range(n_new)]
    assert [pf.host_resample_rank(k, m, n_new) for k in (0, n_new // 2, n_new - 1)] == \
        [rank(k, m, n_new) for k in (0, n_new // 2, n_new - 1)]
    # the properties
    assert source[0] >= 0 and source[-1] < m and np.all(np.diff(source) >= 0)
    if n_new >= m:
        uses = np.bincount(source, minlength=m)
        assert set(uses.tolist()) <= {n_new // m, -(-n_new // m)}
    if n_new < m:
        assert set(np.diff(source).tolist()) <= {m // n_new, -(-m // n_new)}
    if n_new == m:
        assert np.array_equal(source, np.arange(m))


@pytest.mark.parametrize("m,n_new", [(300_001, 1000), (1000, 300_001), (300_001, 300_001)])
def test_rank_properties_at_a_large_count(m, n_new):
    source, members = pf.host_resample_source(None, 0, n_new, N=m)
    k = np.arange(n_new, dtype=np.int64)
    assert members == m and np.array_equal(source, ((2 * k + 1) * m) // (2 * n_new))
    uses = np.bincount(source, minlength=m)
    if n_new >= m:
        assert uses.min() >= n_new // m and uses.max() <= -(-n_new // m)
    else:
        gaps = np.diff(source)
        assert uses.max() == 1 and gaps.min() >= m // n_new and gaps.max() <= -(-m // n_new)


def test_rank_at_the_largest_counts():
    """(2k + 1) m reaches (2^32 - 3)(2^31 - 1) < 2^63: the one-slot probe at both ends and in the middle."""
    for k in (0, 1, BIG // 2, BIG - 2, BIG - 1):
        assert pf.host_resample_rank(k, BIG, BIG) == k == rank(k, BIG, BIG)
        assert pf.host_resample_rank(k, 1, BIG) == 0
    for k, n_new in ((0, 1), (BIG - 1, BIG), (12345, 99991)):
        assert pf.host_resample_rank(k, BIG, n_new) == rank(k, BIG, n_new)


# the member counts of cloud_modes_ref.cloud(300_001, 1)[:N] about cloud_modes_ref.seeds(3), by cloud_modes_ref.assign:
# ungated modes 0 / 1 / 2, then gate 12.0 modes 0 / 1 / 2 and MODE_NONE
COUNTS = {255: ((77, 85, 93), (36, 42, 40, 137)), 4097: ((1325, 1396, 1376), (601, 685, 630, 2181))}


@pytest.mark.parametrize("N", [1, 255, 256, 257, 4097])
def test_members_of_a_mode(N):
    rows, seeds = ref.cloud(300_001, 1)[:N], ref.seeds(3)
    for max_dist in (0.0, 12.0):
        mode_of, counts = pf.host_cloud_assign(rows, seeds, trans_scale=ref.TRANS_SCALE, rot_scale=ref.ROT_SCALE,
                                               max_dist=max_dist)
        if N in COUNTS:
            want = COUNTS[N][1 if max_dist else 0]
            assert tuple(counts[:3]) == want[:3] and counts[3] == (want[3] if max_dist else 0)
        if N == 1:
            assert list(counts) == [0, 1, 0, 0]  # the one particle is mode 1: mode 0 has no member
        for mode, m in zip((0, 1, 2, pf.MODE_NONE), counts):
            members = np.flatnonzero(mode_of == mode)
            assert len(members) == m
            for n_new in sorted({1, max(m - 1, 1), max(m, 1), m + 1, 2 * N}):
                source, got_m = pf.host_resample_source(mode_of, mode, n_new)
                assert got_m == m
                if m == 0:
                    assert len(source) == 0
                    continue
                assert len(source) == n_new and np.all(np.diff(source) >= 0) and np.all(mode_of[source] == mode)
                assert np.array_equal(source, members[[rank(k, m, n_new) for k in range(n_new)]])


def _raw(mode_of, N, mode, n_new, null=()):
    lib = pf.load()
    source = np.full(max(n_new, 0) + 4, -7, dtype=np.int32)
    m = C.c_int64(-9)
    mo = None if mode_of is None else mode_of.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.pfmpe_host_resample_source(mo, N, mode, n_new,
                                        None if "source" in null else source.ctypes.data_as(C.POINTER(C.c_int32)),
                                        None if "n_members" in null else C.byref(m))
    return rc, source, m.value


def test_errors_leave_the_outputs_untouched():
    mode_of = np.array([0, 1, 0], dtype=np.uint8)
    for args, null in (((mode_of, 3, 0, 2), ("source",)), ((mode_of, 3, 0, 2), ("n_members",)), ((mode_of, -1, 0, 2), ()),
                       ((mode_of, 3, 0, -1), ()), ((None, 2**31, 0, 2), ()), ((mode_of, 3, 0, 2**31), ()),
                       ((mode_of, 3, -1, 2), ()), ((mode_of, 3, 256, 2), ())):
        rc, source, m = _raw(*args, null=null)
        assert rc == pf.E_ARG, (args[1:], null)
        assert np.all(source == -7) and m == -9
    # and what is allowed: no slots (a NULL source then), no particles, a mode nobody has, any mode without mode_of
    assert _raw(mode_of, 3, 0, 0, null=("source",))[::2] == (pf.OK, 2)
    assert _raw(None, 0, 0, 3)[::2] == (pf.OK, 0)
    rc, source, m = _raw(mode_of, 3, 7, 3)
    assert (rc, m) == (pf.OK, 0) and np.all(source == -7)  # no member: no source entry written
    rc, source, m = _raw(None, 3, -5, 2)
    assert (rc, m) == (pf.OK, 3) and source[:2].tolist() == [0, 2] and np.all(source[2:] == -7)
    rc, source, m = _raw(mode_of, 3, 0, 3)
    assert (rc, m) == (pf.OK, 2) and source[:3].tolist() == [0, 2, 2] and np.all(source[3:] == -7)
    # the one-slot probe
    lib = pf.load()
    r = C.c_int64(-9)
    for k, mm, n_new in ((0, 0, 1), (0, 1, 0), (-1, 1, 1), (1, 1, 1), (0, 2**31, 1), (0, 1, 2**31)):
        assert lib.pfmpe_host_resample_rank(k, mm, n_new, C.byref(r)) == pf.E_ARG and r.value == -9
    assert lib.pfmpe_host_resample_rank(0, 1, 1, None) == pf.E_ARG
