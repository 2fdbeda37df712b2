"""The host-only companions of pfmpe_assoc_stats_multi (no GPU, no context): pfmpe_host_assoc_plan, the batch's layout,
against a Python restatement of include/pfmpe.h's wording, and pfmpe_host_gate_pairs, the rule of INTEGRATION.md §5f,
against a Python restatement of its definition and against the old §5f snippet at the defaults."""
import ctypes as C

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

MAXM = pf.MAX_MARKERS
LDS_LIMIT = 64 * 1024


# ---------------------------------------------------------------------------------------------- the plan
def align16(x):
    return (x + 15) // 16 * 16


def bucket_count(B):
    nb = 128
    while nb < 512 and nb < 2 * B:
        nb *= 2
    return nb


def table_bytes_no_grid(B, f64):
    """A blob table without a grid (DESIGN.md "Exact blob pruning"): header of 4 T, bstart[nb + 1], xy[B], orig[B],
    each part rounded up to 16 bytes, then the 48-byte grid header and the sentinel entry."""
    t = 8 if f64 else 4
    return align16(4 * t) + align16((bucket_count(B) + 1) * 4) + align16(B * 2 * t) + align16(B * 4) + 48 + 16


def consts_bytes(f64):
    # LdsConst: cur, pred, predm, cam (12 each), 16 x 3 markers, K (9), lo, hi, rgs (6 each)
    return (4 * 12 + 48 + 9 + 18) * (8 if f64 else 4)


def marker_bucket(M):
    return 5 if M == 5 else 8 if M <= 8 else 12 if M <= 12 else 16


def py_plan(N, M, B, which=None, prune=None, table_bytes=None, state=pf.STATE_F32):
    f64 = state == pf.STATE_F64
    plan, keys, launch_blocks, words = [], [], [], 0
    for s in range(len(N)):
        tb = table_bytes[s] if table_bytes is not None else table_bytes_no_grid(B[s], f64)
        bins = M[s] * B[s] + M[s] + 1
        key = ((which[s] if which is not None else pf.ASSOC_POSTERIOR), marker_bucket(M[s]),
               (1 if prune[s] else 0) if prune is not None else 1)
        if key not in keys:
            keys.append(key)
            launch_blocks.append(0)
        l = keys.index(key)
        blocks = min((N[s] + 255) // 256, 1024)
        words = (words + 3) // 4 * 4
        plan.append({"bins_offset": words, "first_block": launch_blocks[l], "blocks": blocks, "launch": l,
                     "lds_votes": 1 if tb + 16 + 4 * bins + consts_bytes(f64) <= LDS_LIMIT else 0})
        words += bins
        launch_blocks[l] += blocks
    return plan, {"bins_words": words, "launches": len(keys), "launch_blocks": launch_blocks}


def test_plan_single_entry():
    plan, total = pf.host_assoc_plan([100000], [5], [50])
    assert plan == [{"bins_offset": 0, "first_block": 0, "blocks": 391, "launch": 0, "lds_votes": 1}]
    assert total == {"bins_words": 5 * 50 + 5 + 1, "launches": 1, "launch_blocks": [391]}
    assert (plan, total) == py_plan([100000], [5], [50])


@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F64, pf.STATE_F16])
def test_plan_block_counts_and_offsets(state):
    N = [1, 255, 256, 257, 262144, 262181]
    M = [5, 4, 5, 12, 16, 5]
    B = [50, 3, 0, 200, 7, 50]
    got = pf.host_assoc_plan(N, M, B, state_dtype=state)
    assert got == py_plan(N, M, B, state=state)
    assert [p["blocks"] for p in got[0]] == [1, 1, 1, 2, 1024, 1024]
    # each start rounded up to 4 words, in index order, entries not overlapping
    end = 0
    for p, m, b in zip(got[0], M, B):
        assert p["bins_offset"] % 4 == 0 and end <= p["bins_offset"] < end + 4
        end = p["bins_offset"] + m * b + m + 1
    assert got[1]["bins_words"] == end


def test_plan_full_batch_and_launch_groups():
    rng = np.random.default_rng(7)
    S = pf.ASSOC_MAX_STREAMS
    N = rng.integers(1, 300000, S).tolist()
    M = rng.integers(1, MAXM + 1, S).tolist()
    B = rng.integers(0, 300, S).tolist()
    which = rng.integers(0, 2, S).tolist()
    prune = rng.integers(0, 2, S).tolist()
    got = pf.host_assoc_plan(N, M, B, which, prune)
    assert got == py_plan(N, M, B, which, prune)
    assert 1 < got[1]["launches"] <= pf.ASSOC_MAX_LAUNCHES
    # a tracker whose objects share M and options: one launch, whatever the particle and blob counts
    one = pf.host_assoc_plan(N, [5] * S, B)
    assert one[1]["launches"] == 1 and one == py_plan(N, [5] * S, B)
    assert one[1]["launch_blocks"] == [sum(min((n + 255) // 256, 1024) for n in N)]


@pytest.mark.parametrize("state", [pf.STATE_F32, pf.STATE_F64])
def test_plan_lds_limit_both_sides(state):
    f64 = state == pf.STATE_F64

    def need(M, B):
        return table_bytes_no_grid(B, f64) + 16 + 4 * (M * B + M + 1) + consts_bytes(f64)

    # the largest B whose bins still fit beside the table for M = 16, and the next one
    B_fit = max(b for b in range(1, 1025) if need(16, b) <= LDS_LIMIT)
    assert B_fit < 1024 and need(16, B_fit + 1) > LDS_LIMIT
    plan, _ = pf.host_assoc_plan([1000, 1000, 1000, 1000], [16, 16, 16, 5], [B_fit, B_fit + 1, 1024, 50],
                                 state_dtype=state)
    assert [p["lds_votes"] for p in plan] == [1, 0, 0, 1]
    # the same decision from a built table's size: a byte more than fits turns the entry to the direct path
    room = LDS_LIMIT - 16 - 4 * (5 * 50 + 5 + 1) - consts_bytes(f64)
    plan, _ = pf.host_assoc_plan([1000, 1000], [5, 5], [50, 50], table_bytes=[room, room + 16], state_dtype=state)
    assert [p["lds_votes"] for p in plan] == [1, 0]


def _raw_plan(N, M, B, S, state=pf.STATE_F32, which=None, tb=None, null=()):
    lib = pf.load()
    arrs = {k: (np.asarray(v, dtype=np.int32) if v is not None else None)
            for k, v in (("N", N), ("M", M), ("B", B), ("which", which), ("tb", tb))}
    ptr = {k: (a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None and k not in null else None)
           for k, a in arrs.items()}
    plan = (_capi.AssocPlan * 65)()
    total = _capi.AssocPlanTotal()
    C.memset(plan, 0xAB, C.sizeof(plan))
    C.memset(C.byref(total), 0xAB, C.sizeof(total))
    rc = lib.pfmpe_host_assoc_plan(ptr["N"], ptr["M"], ptr["B"], ptr["which"], None, ptr["tb"], S, state,
                                   None if "plan" in null else plan, None if "total" in null else C.byref(total))
    untouched = bytes(plan) == b"\xab" * C.sizeof(plan) and bytes(total) == b"\xab" * C.sizeof(total)
    return rc, untouched


def test_plan_errors_leave_outputs_untouched():
    ok = ([1000, 10], [5, 5], [50, 0])
    assert _raw_plan(*ok, 2) == (pf.OK, False)
    for null in ("N", "M", "B", "plan", "total"):
        assert _raw_plan(*ok, 2, null=(null,)) == (pf.E_ARG, True), null
    assert _raw_plan(*ok, 0) == (pf.E_ARG, True)
    assert _raw_plan(*ok, -1) == (pf.E_ARG, True)
    assert _raw_plan(*ok, 2, state=3) == (pf.E_ARG, True)
    assert _raw_plan([1000, 0], [5, 5], [50, 0], 2) == (pf.E_ARG, True)
    assert _raw_plan([1000, 10], [5, 0], [50, 0], 2) == (pf.E_ARG, True)
    assert _raw_plan([1000, 10], [5, MAXM + 1], [50, 0], 2) == (pf.E_ARG, True)
    assert _raw_plan([1000, 10], [5, 5], [50, -1], 2) == (pf.E_ARG, True)
    assert _raw_plan(*ok, 2, which=[1, 2]) == (pf.E_ARG, True)
    assert _raw_plan(*ok, 2, tb=[1000, -16]) == (pf.E_ARG, True)
    # capacity
    assert _raw_plan([10] * 65, [5] * 65, [1] * 65, 65) == (pf.E_CAP, True)
    assert _raw_plan([10] * 64, [5] * 64, [1] * 64, 64) == (pf.OK, False)
    assert _raw_plan([1000, 10], [5, 5], [50, pf.MAX_BLOBS + 1], 2) == (pf.E_CAP, True)
    assert _raw_plan(*ok, 2, tb=[1000, LDS_LIMIT]) == (pf.E_CAP, True)  # a table that does not fit the LDS at all
    with pytest.raises(pf.PFError):
        pf.host_assoc_plan([0], [5], [5])


# ---------------------------------------------------------------------------------------------- the gate
def py_summary(votes):
    """(mode_blob, mode_votes, second_votes) per LED as pfmpe_host_assoc_summary forms them: a strict test keeps the
    lowest blob index among equal counts; mode_blob 0 when no particle matched the LED."""
    res = []
    for row in votes:
        best = second = arg = 0
        for b in range(1, len(row)):
            if row[b] > best:
                second, best, arg = best, int(row[b]), b
            elif row[b] > second:
                second = int(row[b])
        res.append((arg if best else 0, best, second))
    return res


def py_gate(votes, pairs, min_share=0.5, lead=2.0, min_pairs=4):
    votes = np.asarray(votes, dtype=np.uint32)
    n = int(votes[0].sum())
    summ = py_summary(votes)
    reason, kept = [], []
    for led, blob in pairs:
        v = int(votes[led - 1][blob])
        mode_blob, mode_votes, second_votes = summ[led - 1]
        r = 0
        if not (float(v) >= min_share * float(n)):
            r |= 1
        if mode_blob != blob:
            r |= 2
        if lead * float(second_votes) > float(mode_votes):
            r |= 4
        reason.append(r)
        if r == 0:
            kept.append((led, blob))
    fallback = 1 if len(kept) < min_pairs else 0
    rows = list(pairs) if fallback else kept
    gated = np.zeros((MAXM, 2), dtype=np.uint32)
    if rows:
        gated[: len(rows)] = rows
    return {"n_in": len(pairs), "n_gated": len(kept), "fallback": fallback, "reason": reason, "gated": gated}


def old_snippet(votes, as_, corr, n_corr, min_num_leds):
    """INTEGRATION.md §5f as it stood before pfmpe_host_gate_pairs, transcribed: the share as a quotient, the lead as
    an integer product."""
    B = votes.shape[1] - 1
    flat = votes.reshape(-1)
    gated = []
    for k in range(n_corr):
        led, blob = int(corr[2 * k]), int(corr[2 * k + 1])
        share = float(flat[(led - 1) * (B + 1) + blob]) / float(as_["n"])
        contested = int(as_["mode_blob"][led - 1]) != blob or \
            2 * int(as_["second_votes"][led - 1]) > int(as_["mode_votes"][led - 1])
        if share >= 0.5 and not contested:
            gated.append((led, blob))
    return gated, len(gated) >= min_num_leds


def check(votes, pairs, **kw):
    got = pf.host_gate_pairs(votes, pairs, **kw)
    want = py_gate(votes, pairs, **kw)
    assert got["n_in"] == want["n_in"] and got["n_gated"] == want["n_gated"] and got["fallback"] == want["fallback"]
    assert got["reason"].tolist() == want["reason"]
    assert np.array_equal(got["gated"], want["gated"])
    return got


def random_table(rng, M, B, n):
    """An (M, B + 1) table whose rows each sum to n, with a clear mode in some rows and near ties in others."""
    votes = np.zeros((M, B + 1), dtype=np.uint32)
    for m in range(M):
        if B == 0:
            votes[m, 0] = n
            continue
        style = rng.integers(0, 4)
        if style == 0:      # spread
            p = rng.dirichlet(np.ones(B + 1))
        elif style == 1:    # one strong blob
            p = np.full(B + 1, 0.1 / (B + 1))
            p[rng.integers(1, B + 1)] += 0.9
        elif style == 2:    # two contenders
            p = np.full(B + 1, 0.05 / (B + 1))
            a, b = rng.integers(1, B + 1, 2)
            p[a] += 0.55
            p[b] += 0.40
        else:               # mostly unpaired
            p = np.full(B + 1, 0.2 / (B + 1))
            p[0] += 0.8
        votes[m] = rng.multinomial(n, p / p.sum())
    return votes


def random_pairs(rng, votes):
    M, B = votes.shape[0], votes.shape[1] - 1
    if B == 0:
        return []
    leds = rng.permutation(M)[: rng.integers(0, M + 1)] + 1
    modes = py_summary(votes)
    pairs = []
    for led in leds:  # mostly the LED's mode, sometimes another blob
        mb = modes[led - 1][0]
        blob = mb if (mb and rng.random() < 0.7) else int(rng.integers(1, B + 1))
        pairs.append((int(led), blob))
    return pairs


def test_gate_random_tables_match_definition_and_old_snippet():
    rng = np.random.default_rng(2024)
    kept_some = fell_back = 0
    for case in range(200):
        M = int(rng.integers(1, MAXM + 1))
        B = int(rng.integers(0, 41))
        n = int(rng.integers(1, 5000))
        votes = random_table(rng, M, B, n)
        pairs = random_pairs(rng, votes)
        got = check(votes, pairs)
        # the old snippet at the defaults: the same kept rows and the same decision
        row = np.zeros(2 * MAXM, dtype=np.uint32)
        row[: 2 * len(pairs)] = np.asarray(pairs, dtype=np.uint32).reshape(-1)
        kept, enough = old_snippet(votes, pf.host_assoc_summary(votes), row, len(pairs), 4)
        assert got["n_gated"] == len(kept) and got["fallback"] == (0 if enough else 1)
        if enough:
            assert got["gated"][: len(kept)].tolist() == [list(p) for p in kept] and not got["gated"][len(kept):].any()
        else:
            assert got["gated"].reshape(-1).tolist() == row.tolist()
        kept_some += got["n_gated"] > 0
        fell_back += got["fallback"]
        # other parameters, against the definition
        check(votes, pairs, min_share=float(rng.random()), lead=float(rng.random() * 4), min_pairs=int(rng.integers(0, 6)))
    assert kept_some > 40 and 40 < fell_back < 200  # both outcomes are exercised


def test_gate_ties_of_mode_and_runner_up():
    # LED 1: blobs 2 and 3 tie at 40: the mode is the lower index, the runner-up has as many votes
    votes = np.array([[20, 0, 40, 40], [10, 90, 0, 0]], dtype=np.uint32)
    got = check(votes, [(1, 2), (1, 3), (2, 1)], min_pairs=0)
    assert got["reason"].tolist() == [1 | 4, 1 | 2 | 4, 0]
    got = check(votes, [(1, 2)], min_pairs=0, min_share=0.4, lead=1.0)  # a lead of 1 accepts the tie
    assert got["reason"].tolist() == [0] and got["gated"][0].tolist() == [1, 2]
    got = check(votes, [(1, 3)], min_pairs=0, min_share=0.4, lead=1.0)  # but blob 3 is not the mode
    assert got["reason"].tolist() == [2]


def test_gate_share_and_lead_exactly_at_their_thresholds():
    # v exactly min_share * n (kept: the test is >=), and one vote less
    votes = np.array([[50, 50, 0], [51, 49, 0]], dtype=np.uint32)
    got = check(votes, [(1, 1), (2, 1)], min_pairs=0)
    assert got["reason"].tolist() == [0, 1]
    # second exactly mode / lead (kept: the test is >), and one vote more
    votes = np.array([[10, 60, 30], [9, 60, 31]], dtype=np.uint32)
    got = check(votes, [(1, 1), (2, 1)], min_pairs=0)
    assert got["reason"].tolist() == [0, 4]
    # thresholds that are not exact in binary, against the same double arithmetic
    votes = np.array([[70, 30, 0], [71, 29, 0]], dtype=np.uint32)
    got = check(votes, [(1, 1), (2, 1)], min_pairs=0, min_share=0.3, lead=0.0)
    assert got["reason"].tolist() == [0 if 30.0 >= 0.3 * 100.0 else 1, 1]


def test_gate_led_nobody_matched_and_empty_table():
    votes = np.array([[100, 0, 0], [0, 100, 0]], dtype=np.uint32)
    got = check(votes, [(1, 1), (2, 1)], min_pairs=0)
    assert got["reason"].tolist() == [1 | 2, 0]  # mode_blob 0 != 1; 2 * 0 > 0 is false
    # min_share 0 lets a pair without votes pass the share test; it is still not the mode
    got = check(votes, [(1, 2)], min_pairs=0, min_share=0.0)
    assert got["reason"].tolist() == [2]
    # n = 0 (an all-zero table): v >= 0.5 * 0 holds, no LED has a mode
    got = check(np.zeros((2, 3), dtype=np.uint32), [(1, 1)], min_pairs=0)
    assert got["reason"].tolist() == [2]


def test_gate_fallback_at_min_pairs():
    votes = np.zeros((6, 4), dtype=np.uint32)
    votes[:, 1] = 100
    votes[3:, 1], votes[3:, 0] = 10, 90  # LEDs 4-6 are mostly unpaired
    pairs = [(1, 1), (4, 1), (2, 1), (3, 1), (5, 1)]
    got = check(votes, pairs)  # 3 kept < 4: the input row unchanged
    assert (got["n_gated"], got["fallback"]) == (3, 1)
    assert got["gated"][:5].tolist() == [list(p) for p in pairs] and not got["gated"][5:].any()
    got = check(votes, pairs, min_pairs=3)  # n_gated = min_pairs: gated, in order, zero padded
    assert (got["n_gated"], got["fallback"]) == (3, 0)
    assert got["gated"][:3].tolist() == [[1, 1], [2, 1], [3, 1]] and not got["gated"][3:].any()
    assert check(votes, pairs, min_pairs=4)["fallback"] == 1
    assert check(votes, pairs, min_pairs=0)["fallback"] == 0


def test_gate_no_pairs_and_defaults():
    p = pf.default_gate_params()
    assert (p.min_share, p.lead, p.min_pairs) == (0.5, 2.0, 4)
    votes = np.array([[0, 10], [0, 10]], dtype=np.uint32)
    got = check(votes, [])
    assert (got["n_in"], got["n_gated"], got["fallback"]) == (0, 0, 1) and not got["gated"].any()
    assert check(votes, [], min_pairs=0)["fallback"] == 0
    # B = 0: a table of one column takes no pair at all
    assert check(np.array([[7], [7]], dtype=np.uint32), [])["n_in"] == 0
    # NULL params are the defaults
    lib = pf.load()
    u32 = C.POINTER(C.c_uint32)
    row = np.zeros(2 * MAXM, dtype=np.uint32)
    row[:2] = (1, 1)
    gated = np.zeros(2 * MAXM, dtype=np.uint32)
    out = _capi.GateOut()
    assert lib.pfmpe_host_gate_pairs(votes.ctypes.data_as(u32), 2, 1, row.ctypes.data_as(u32), 1, None,
                                     gated.ctypes.data_as(u32), C.byref(out)) == pf.OK
    assert (out.n_in, out.n_gated, out.fallback) == (1, 1, 1) and gated.tolist() == row.tolist()


def _raw_gate(votes, M, B, row, n_corr, prm=None, null=()):
    lib = pf.load()
    u32 = C.POINTER(C.c_uint32)
    votes = np.ascontiguousarray(votes, dtype=np.uint32)
    row = np.ascontiguousarray(row, dtype=np.uint32)
    gated = np.full(2 * MAXM, 0xABABABAB, dtype=np.uint32)
    out = _capi.GateOut()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    rc = lib.pfmpe_host_gate_pairs(None if "votes" in null else votes.ctypes.data_as(u32), M, B,
                                   None if "corr" in null else row.ctypes.data_as(u32), n_corr,
                                   C.byref(prm) if prm is not None else None,
                                   None if "gated" in null else gated.ctypes.data_as(u32),
                                   None if "out" in null else C.byref(out))
    untouched = bool((gated == 0xABABABAB).all()) and bytes(out) == b"\xab" * C.sizeof(out)
    return rc, untouched


def test_gate_errors_leave_outputs_untouched():
    votes = np.array([[10, 80, 10], [10, 10, 80]], dtype=np.uint32)
    row = np.zeros(2 * MAXM, dtype=np.uint32)
    row[:4] = (1, 1, 2, 2)
    assert _raw_gate(votes, 2, 2, row, 2) == (pf.OK, False)
    for null in ("votes", "corr", "gated", "out"):
        assert _raw_gate(votes, 2, 2, row, 2, null=(null,)) == (pf.E_ARG, True), null
    assert _raw_gate(votes, 0, 2, row, 2) == (pf.E_ARG, True)
    assert _raw_gate(votes, MAXM + 1, 2, row, 2) == (pf.E_ARG, True)
    assert _raw_gate(votes, 2, -1, row, 2) == (pf.E_ARG, True)
    assert _raw_gate(votes, 2, pf.MAX_BLOBS + 1, row, 2) == (pf.E_ARG, True)
    assert _raw_gate(votes, 2, 2, row, -1) == (pf.E_ARG, True)
    assert _raw_gate(votes, 2, 2, np.ones(2 * MAXM + 2, dtype=np.uint32), MAXM + 1) == (pf.E_ARG, True)
    for bad in ((0, 1), (3, 1), (1, 0), (1, 3)):  # an LED outside 1..M, a blob outside 1..B
        r = row.copy()
        r[2:4] = bad
        assert _raw_gate(votes, 2, 2, r, 2) == (pf.E_ARG, True), bad
        assert _raw_gate(votes, 2, 2, r, 1) == (pf.OK, False), bad  # beyond n_corr the row is not read
    uneven = votes.copy()
    uneven[1, 0] += 1
    assert _raw_gate(uneven, 2, 2, row, 2) == (pf.E_ARG, True)  # rows that do not all sum to n
    for field, val in (("min_share", float("nan")), ("min_share", -0.1), ("min_share", float("inf")),
                       ("lead", float("nan")), ("lead", -1.0), ("lead", float("inf")), ("min_pairs", -1)):
        prm = pf.default_gate_params()
        setattr(prm, field, val)
        assert _raw_gate(votes, 2, 2, row, 2, prm) == (pf.E_ARG, True), (field, val)
    with pytest.raises(pf.PFError):
        pf.host_gate_pairs(votes, [(3, 1)])
