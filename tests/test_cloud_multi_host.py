"""Host side of the batch cloud statistics (pfmpe_cloud_stats_multi): the binding's symbols and record sizes, and the
grid the batch launches (pfmpe_host_cloud_plan): each entry's block count is its single call's, the prefix sums, the
largest batch, and the error cases.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

BLOCK, MAX_BLOCKS = 256, 1024


def test_symbols_and_sizes():
    for name in ("pfmpe_cloud_stats_multi", "pfmpe_host_cloud_plan"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(pf.load(), name)
    assert C.sizeof(pf.CloudIn) == 104
    assert C.sizeof(pf.CloudPlan) == 8
    assert C.sizeof(pf.CloudOut) == 480
    assert _capi.CLOUD_MAX_STREAMS == 64 == pf.CLOUD_MAX_STREAMS
    assert hasattr(pf.Engine, "cloud_stats_multi")
    assert pf.CloudIn.which.offset == 96


def test_header_declares_them():
    import os
    hdr = open(os.path.join(os.path.dirname(_capi.__file__), "..", "include", "pfmpe.h")).read()
    assert "#define PFMPE_CLOUD_MAX_STREAMS 64" in hdr
    assert ("int pfmpe_cloud_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, "
            "pfmpe_cloud_out* out);") in hdr
    assert "int pfmpe_host_cloud_plan(const int32_t* N, int S, pfmpe_cloud_plan* plan, int32_t* total_blocks);" in hdr


def test_plan_block_counts_and_prefix():
    """one particle, a block less one, a block, a block plus one, the last N with a block per 256 particles, the first
    that strides, and far beyond"""
    Ns = [1, 255, 256, 257, 262_144, 262_145, 10_000_000]
    plan, total = pf.host_cloud_plan(Ns)
    assert [p["blocks"] for p in plan] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert [p["first_block"] for p in plan] == [0, 1, 2, 3, 5, 1029, 2053]
    assert total == 3077


def test_plan_is_the_single_calls_grid():
    rng = np.random.default_rng(5)
    for _ in range(50):
        S = int(rng.integers(1, 65))
        Ns = rng.integers(1, 600_000, size=S).tolist()
        plan, total = pf.host_cloud_plan(Ns)
        nxt = 0
        for n, p in zip(Ns, plan):
            assert p["blocks"] == min(-(-n // BLOCK), MAX_BLOCKS)
            assert p["first_block"] == nxt
            nxt += p["blocks"]
        assert total == nxt


def test_largest_batch():
    plan, total = pf.host_cloud_plan([3 + 5 * i for i in range(64)])
    assert len(plan) == 64 and total == sum(p["blocks"] for p in plan)
    plan, total = pf.host_cloud_plan([2**31 - 1] * 64)
    assert total == 64 * MAX_BLOCKS and plan[63]["first_block"] == 63 * MAX_BLOCKS


def _raw(Ns, S=None, null_n=False, null_plan=False, null_total=False):
    n = np.ascontiguousarray(Ns, dtype=np.int32)
    S = len(Ns) if S is None else S
    plan = (_capi.CloudPlan * max(len(Ns), 1))(*[_capi.CloudPlan(-7, -7) for _ in range(max(len(Ns), 1))])
    total = C.c_int32(-7)
    i32 = C.POINTER(C.c_int32)
    rc = pf.load().pfmpe_host_cloud_plan(None if null_n else n.ctypes.data_as(i32), S, None if null_plan else plan,
                                         None if null_total else C.byref(total))
    untouched = total.value == -7 and all(p.first_block == -7 and p.blocks == -7 for p in plan)
    return rc, untouched


def test_plan_errors_leave_the_outputs_untouched():
    assert _raw([100, 200])[0] == pf.OK and not _raw([100, 200])[1]
    for name, (rc, untouched), code in [
        ("S = 0", _raw([100, 200], S=0), pf.E_ARG),
        ("S < 0", _raw([100, 200], S=-1), pf.E_ARG),
        ("null N", _raw([100, 200], null_n=True), pf.E_ARG),
        ("null plan", _raw([100, 200], null_plan=True), pf.E_ARG),
        ("null total", _raw([100, 200], null_total=True), pf.E_ARG),
        ("N = 0", _raw([100, 200, 0]), pf.E_ARG),
        ("N < 0", _raw([100, -5, 300]), pf.E_ARG),
        ("S = 65", _raw([100] * 65), pf.E_CAP),
    ]:
        assert rc == code, (name, rc)
        assert untouched, name
    with pytest.raises(pf.PFError) as e:
        pf.host_cloud_plan([10, 0])
    assert e.value.code == pf.E_ARG
    with pytest.raises(pf.PFError) as e:
        pf.host_cloud_plan([10] * 65)
    assert e.value.code == pf.E_CAP


def test_binding_rejects_length_mismatch_before_any_call():
    class NoCtx:  # never reached: the lengths are checked first
        pass
    with pytest.raises(ValueError):
        pf.Engine.cloud_stats_multi([NoCtx(), NoCtx()], [pf.CLOUD_POSTERIOR], [np.eye(4), np.eye(4)])
    with pytest.raises(ValueError):
        pf.Engine.cloud_stats_multi([NoCtx()], [pf.CLOUD_POSTERIOR], [])
    with pytest.raises(ValueError):
        pf.Engine.cloud_stats_multi([], [], [])
    ci = pf.Engine.make_cloud_in(pf.CLOUD_WEIGHTED, np.arange(16.0).reshape(4, 4))
    assert list(ci.ref_pose) == list(range(12)) and ci.which == pf.CLOUD_WEIGHTED and ci.pad == 0
