"""Host side of the batch initialisation (pfmpe_initialise_multi): the binding's symbols and record sizes, and the
work mapping of its histogram stage (pfmpe_host_init_plan): the plan's invariants over mixed batches, the coverage of
a stream's items by its blocks, the LDS threshold, and the error cases.  No GPU."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

BLOCK = 256


def items_of(M, B):
    return comb(B, 3) * M * (M - 1) * (M - 2) if B >= M and B >= 3 else 0


def bucket_of(M):
    return 0 if M - 3 <= 2 else 1 if M - 3 <= 9 else 2


def test_symbols_and_sizes():
    for name in ("pfmpe_initialise_multi", "pfmpe_host_init_plan"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(pf.load(), name)
    assert C.sizeof(pf.InitPlan) == 24
    assert C.sizeof(pf.InitIn) == 16
    assert _capi.INIT_MAX_STREAMS == 64 == pf.INIT_MAX_STREAMS
    assert hasattr(pf.Engine, "initialise_multi")


def mixed_batches():
    rng = np.random.default_rng(11)
    yield [5], [8]
    yield [5, 5, 8, 6, 5, 5], [8, 17, 11, 11, 4, 9]
    yield [3, 4, 5, 6, 12, 13, 16], [0, 3, 60, 60, 60, 12, 16]
    yield [16] * 64, [60] * 64
    yield [5] * 64, [5] * 64
    for _ in range(40):
        S = int(rng.integers(1, 65))
        yield rng.integers(3, 17, size=S).tolist(), rng.integers(0, 61, size=S).tolist()


@pytest.mark.parametrize("num_cu", [1, 4, 256])
def test_plan_invariants(num_cu):
    cap = 8 * num_cu
    hit = 0
    for M, B in mixed_batches():
        plan, per_bucket = pf.host_init_plan(M, B, num_cu)
        assert len(plan) == len(M)
        nxt, wants, with_work = [0, 0, 0], [0, 0, 0], [0, 0, 0]
        for m, b, p in zip(M, B, plan):
            it = items_of(m, b)
            assert p["items"] == it
            assert p["bucket"] == bucket_of(m)
            assert p["lds_hist"] == (1 if b * m * 4 <= 32768 else 0)
            assert p["first_block"] == nxt[p["bucket"]]  # the running sum, ascending stream index
            want = -(-it // BLOCK)
            if it == 0:
                assert p["blocks"] == 0
            else:
                assert 1 <= p["blocks"] <= want
                with_work[p["bucket"]] += 1
            nxt[p["bucket"]] += p["blocks"]
            wants[p["bucket"]] += want
        assert per_bucket == nxt
        for k in range(3):
            if wants[k] <= cap:  # nothing is scaled: every stream has what it wants
                assert per_bucket[k] == wants[k]
            else:
                hit += 1
                # the cap holds except for the one-block minimum: the streams above one block fit under it, and the
                # launch is over it by less than one block per stream with work
                above = sum(p["blocks"] for p in plan if p["bucket"] == k and p["blocks"] > 1)
                assert above <= cap
                assert per_bucket[k] <= cap + with_work[k]
                # proportional: a stream's share is floor(want * cap / wants), at least 1
                for m, b, p in zip(M, B, plan):
                    if p["bucket"] == k and p["items"]:
                        assert p["blocks"] == max(1, -(-p["items"] // BLOCK) * cap // wants[k])
    assert hit > 0  # the scaled branch was exercised


def test_plan_is_deterministic():
    M, B = [5, 8, 16, 5, 9], [50, 20, 16, 8, 30]
    assert pf.host_init_plan(M, B, 4) == pf.host_init_plan(M, B, 4)


@pytest.mark.parametrize("num_cu", [1, 256])
def test_blocks_visit_every_item_once(num_cu):
    """Block b (of `blocks`) of a stream visits b * 256 + t + k * blocks * 256: every item exactly once."""
    shapes = [(3, 3), (4, 5), (5, 8)]
    plan, _ = pf.host_init_plan([m for m, _ in shapes], [b for _, b in shapes], num_cu)
    for (m, b), p in zip(shapes, plan):
        items, blocks = p["items"], p["blocks"]
        assert items == items_of(m, b) > 0 and blocks >= 1
        seen = np.zeros(items, dtype=np.int64)
        rounds = -(-items // (blocks * BLOCK))
        bl, t, k = np.meshgrid(np.arange(blocks), np.arange(BLOCK), np.arange(rounds), indexing="ij")
        visit = (bl * BLOCK + t + k * blocks * BLOCK).ravel()
        np.add.at(seen, visit[visit < items], 1)
        assert (seen == 1).all()


def test_lds_threshold():
    # B * M * 4 <= 32768 keeps the histogram in LDS: M = 16 flips between B = 512 and 513, M = 8 at 1024
    plan, _ = pf.host_init_plan([16, 16, 8, 9], [512, 513, 1024, 911], 256)
    assert [p["lds_hist"] for p in plan] == [1, 0, 1, 0]
    assert 911 * 9 * 4 > 32768 >= 910 * 9 * 4


def test_error_codes():
    lib = pf.load()
    i32 = C.POINTER(C.c_int32)
    plan = (pf.InitPlan * 64)()
    per = (C.c_int32 * 3)(7, 7, 7)

    def call(M, B, S=None, num_cu=4, plan_=plan, per_=per, null_m=False, null_b=False):
        m, b = np.asarray(M, np.int32), np.asarray(B, np.int32)
        return lib.pfmpe_host_init_plan(None if null_m else m.ctypes.data_as(i32),
                                        None if null_b else b.ctypes.data_as(i32), len(M) if S is None else S, num_cu,
                                        plan_, per_)

    assert call([5], [8]) == pf.OK and list(per) == [14, 0, 0]  # 3,360 items
    per[:] = [7, 7, 7]
    for rc in (call([5], [8], null_m=True), call([5], [8], null_b=True), call([5], [8], plan_=None),
               call([5], [8], per_=None), call([5], [8], S=0), call([5] * 65, [8] * 65), call([2], [8]),
               call([17], [20]), call([5], [-1]), call([5, 5], [8, -3])):
        assert rc == pf.E_ARG
    assert call([5], [1025]) == pf.E_CAP  # above PFMPE_MAX_BLOBS
    assert list(per) == [7, 7, 7]  # untouched on every error
    assert call([5] * 64, [8] * 64) == pf.OK
    assert call([5], [8], num_cu=0) == pf.OK and list(per) == [8, 0, 0]  # max(num_cu, 1): the cap of one CU
    with pytest.raises(pf.PFError):
        pf.host_init_plan([5], [-1], 4)
