"""Host side of the batch refinement (pfmpe_refine_multi): the binding's symbols, record sizes and constants, and the
packed upload buffer (pfmpe_host_refine_plan): prefix sums, alignment, disjointness and containment of its regions,
their sizes, determinism, and the error cases.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

KS = (0, 1, 65, 300)
BS = (0, 1, 12, 40)
MODEL_BYTES = 8 * (3 * pf.MAX_MARKERS + 9)


def test_symbols_sizes_and_constants():
    for name in ("pfmpe_refine_multi", "pfmpe_host_refine_plan"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(pf.load(), name)
    assert C.sizeof(pf.RefineIn) == 40
    assert C.sizeof(pf.RefinePlan) == 24
    assert C.sizeof(pf.RefinePlanTotal) == 56
    assert C.sizeof(pf.RefineOut) == 480 and C.sizeof(pf.RefineRow) == 128
    assert _capi.REFINE_MAX_STREAMS == 64 == pf.REFINE_MAX_STREAMS
    assert _capi.REFINE_MULTI_MAX_HYPOTHESES == 65536 == pf.REFINE_MULTI_MAX_HYPOTHESES
    assert pf.REFINE_DESC_BYTES == 48
    assert hasattr(pf.Engine, "refine_multi")


def batches():
    """(K, B) per stream for S = 1, 3 and 64, K from KS and B from BS."""
    for k, b in itertools.product(KS, BS):
        yield [k], [b]
    rng = np.random.default_rng(5)
    yield [1, 65, 300], [20, 12, 40]
    yield [0, 0, 0], [0, 0, 0]
    yield [300, 0, 1], [0, 40, 1]
    for _ in range(20):
        yield rng.choice(KS, size=3).tolist(), rng.choice(BS, size=3).tolist()
    yield [1] * 64, [12] * 64
    yield [0] * 64, [0] * 64
    yield [300] * 64, [40] * 64
    yield [1, 0] * 32, [40, 0] * 32
    for _ in range(10):
        yield rng.choice(KS, size=64).tolist(), rng.choice(BS, size=64).tolist()


def test_plan_invariants():
    seen_s = set()
    for K, B in batches():
        S = len(K)
        seen_s.add(S)
        plan, tot = pf.host_refine_plan(K, B)
        H = sum(K)
        assert len(plan) == S
        assert tot["hypotheses"] == H
        assert [p["first"] for p in plan] == [sum(K[:s]) for s in range(S)]  # exclusive prefix sum
        # (offset, least size) of every region
        regions = [(tot["desc_offset"], S * pf.REFINE_DESC_BYTES), (tot["stream_of_offset"], 4 * H),
                   (tot["poses_offset"], 96 * H), (tot["corr_offset"], 128 * H)]
        for p, b in zip(plan, B):
            regions.append((p["model_offset"], MODEL_BYTES))
            regions.append((p["blobs_offset"], 16 * b))
        up = tot["upload_bytes"]
        for off, size in regions:
            assert off % 16 == 0, (K, B, off)
            assert 0 <= off and off + size <= up, (K, B, off, size, up)
            assert off < up  # also a region without content lies inside
        # pairwise disjoint: sorted by offset, each ends before the next begins (empty regions take no room)
        filled = sorted(r for r in regions if r[1] > 0)
        for (o1, s1), (o2, _) in zip(filled, filled[1:]):
            assert o1 + s1 <= o2, (K, B, o1, s1, o2)
        assert tot["download_bytes"] == S * C.sizeof(pf.RefineOut) + H * (C.sizeof(pf.RefineRow) + 36 * 8)
        assert pf.host_refine_plan(K, B) == (plan, tot)  # the same inputs, the same plan
    assert seen_s == {1, 3, 64}


def test_layout_depends_on_shapes_alone():
    a = pf.host_refine_plan([1, 65, 300], [20, 12, 40])
    b = pf.host_refine_plan(np.array([1, 65, 300], dtype=np.int64), (20, 12, 40))
    assert a == b
    # another K moves what follows it
    c = pf.host_refine_plan([1, 66, 300], [20, 12, 40])
    assert c[0][2]["first"] == a[0][2]["first"] + 1 and c[1]["upload_bytes"] > a[1]["upload_bytes"]


def test_error_codes():
    lib = pf.load()
    i32 = C.POINTER(C.c_int32)
    plan = (pf.RefinePlan * 66)()
    tot = pf.RefinePlanTotal()
    pattern = 0x5A

    def prefill():
        C.memset(plan, pattern, C.sizeof(plan))
        C.memset(C.byref(tot), pattern, C.sizeof(tot))

    def untouched():
        return bytes(plan) == bytes([pattern]) * C.sizeof(plan) and bytes(tot) == bytes([pattern]) * C.sizeof(tot)

    def call(K, B, S=None, plan_=plan, tot_=C.byref(tot), null_k=False, null_b=False):
        k, b = np.asarray(K, np.int32), np.asarray(B, np.int32)
        return lib.pfmpe_host_refine_plan(None if null_k else k.ctypes.data_as(i32),
                                          None if null_b else b.ctypes.data_as(i32), len(K) if S is None else S, plan_,
                                          tot_)

    prefill()
    cases = [
        (call([1], [8], S=0), pf.E_ARG),
        (call([1] * 65, [8] * 65), pf.E_CAP),
        (call([-1], [8]), pf.E_ARG),
        (call([1, 1, -1], [8, 8, 8]), pf.E_ARG),
        (call([1], [-1]), pf.E_ARG),
        (call([1], [pf.MAX_BLOBS + 1]), pf.E_CAP),
        (call([65536, 1], [8, 8]), pf.E_CAP),  # 65,537 in all
        (call([1025] * 63 + [962], [8] * 64), pf.E_CAP),  # 65,537 over 64 streams
        (call([1], [8], null_k=True), pf.E_ARG),
        (call([1], [8], null_b=True), pf.E_ARG),
        (call([1], [8], plan_=None), pf.E_ARG),
        (call([1], [8], tot_=None), pf.E_ARG),
    ]
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want)
    assert 1025 * 63 + 962 == 65537
    assert untouched()  # the outputs are untouched on every error
    # the limits themselves are accepted
    assert call([65536], [pf.MAX_BLOBS]) == pf.OK and tot.hypotheses == 65536
    assert call([1024] * 64, [pf.MAX_BLOBS] * 64) == pf.OK and tot.hypotheses == 65536
    with pytest.raises(pf.PFError) as e:
        pf.host_refine_plan([1], [-1])
    assert e.value.code == pf.E_ARG


def test_null_contexts_are_refused_without_a_gpu():
    lib = pf.load()
    ins = (pf.RefineIn * 1)()
    outs = (pf.RefineOut * 1)()
    assert lib.pfmpe_refine_multi(None, 1, ins, None, outs, None, None) == pf.E_ARG
    ctxs = (C.c_void_p * 1)(None)
    assert lib.pfmpe_refine_multi(ctxs, 1, ins, None, outs, None, None) == pf.E_ARG
    assert not any(bytes(outs))  # nothing was written
