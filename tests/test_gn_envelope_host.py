"""pfmpe_host_optimise_pose (the code a lane of k_refine runs) against the oracle's optimisePose over the case list of
gn_cases.py.  No GPU.

refine_ref.py decides from a pair count whether a row's pose is determined (MIN_DETERMINED = 3).  That holds for its
three clouds and not beyond them: with 16 LEDs, 40 heavy blobs, initial_prior(truth_pose(3.0), 200) and the oracle's
pairs, rows 25 and 132 have 3 pairs and the oracle and the host alike "converge" 1e34 m away with an rms_after of
13-24 px; the oracle's own result moves by 1e34-1e48 m when the start pose moves one ulp (scaled condition number of A:
8e6).  Both sides are right and a pair count would fail them.  So here the rule of a row comes from the oracle alone:
optimise_pose at the start pose and at nextafter(+-inf) of it, as rr.oracle_refine does, and then

  stable       all runs converge and their poses agree within 1e-12 in every entry: the host must report
               CONVERGED, its pose must be within rr.POSE_BAR (1e-9 m / 1e-9 rad, the project's bar) and, with at
               least 4 pairs, its covariance within rr.COV_MARGIN x the oracle's own largest relative change under
               +-1 ulp over the case's stable rows;
  cap-stable   all runs stop at 500: the host must report a cap status with iters == 500, and CAP_REVERTED
               exactly when all oracle runs returned their start pose's bytes;
  other        only what the iteration does not touch: n_pairs, rms_before, rms_after against numpy at the row's own
               returned pose (relative 1e-9) and the status accounting.

The last line holds for every row of every case, the cases with other parameters than the oracle's included.

The probe is wider than +-1 ulp: the start pose is also moved by 2, 4 and 8 ulps each way (PROBE_ULPS, nine runs), and
a row is stable or cap-stable only if all nine agree.  Three runs were not enough: the host's arithmetic differs from
the oracle's by more than one input ulp (its own sin / cos, the order of sums; rr.COV_MARGIN is 1000 for that reason).
Measured with three runs: row 228 of t0.5-M12 (3 pairs, the object behind the camera) has two exact solutions, 1.35 m
and 2.3 rad apart; the oracle's three runs reach one in 35, 25 and 38 iterations, the host the other in 41 (and the
oracle's one from the +1 ulp start).  Rows 164 and 177 of far-M12 run away to 1e18-1e42 m on both sides; the oracle's
three runs stop at the cap 1e3-1e8 m apart from one another, the host "converges" after 74 and 71 iterations, and
after 500, 407 / 242, 436 from the +-1 ulp starts.  Both sides are right on all three; nine runs put them under
"other", and every row that nine runs call stable three runs call stable too.

The shares: in each bucket case, each K case and the 1.7 scene at least 90 % of the rows whose A can have full rank
(3 pairs or more) are stable or cap-stable; at 0.5 with 4 and 5 LEDs at least a quarter of the rows with pairs are
cap-stable.  The first share cannot be taken over all rows with pairs: in the light cases 25-53 % of them have one or
two pairs (the cloud is +-35 mm wide, a pair needs 5 px), A has rank 2 or 4 there and the oracle's own result moves by
1e30-1e60 m under one ulp (refine_ref.py), whatever the blob seed or the scene time.  Over all rows with pairs the
share is 0.43-0.75 light and 0.95-1.0 heavy; the test prints both.  With 1 or 2 LEDs every row is of that kind.
"""
import functools

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from oracle import pforacle as orc

import gn_cases as gc
import refine_ref as rr

STABLE_TOL = 1e-12
PROBE_ULPS = (1, 2, 4, 8)
STABLE, CAP_STABLE, OTHER, NO_PAIRS = 0, 1, 2, 3
CAPS = (pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED)


@functools.lru_cache(maxsize=None)
def classify(cid):
    """The oracle over a case: per row the class, the pose and covariance of the unperturbed run, whether all three
    runs returned their start pose, and the case's covariance spread over its stable rows with at least 4 pairs."""
    c = gc.case_by_id(cid)
    n = len(c.poses)
    cls = np.full(n, NO_PAIRS)
    pose, cov = np.zeros((n, 12)), np.zeros((n, 6, 6))
    reverted = np.zeros(n, dtype=bool)
    spread = 0.0
    for i in range(n):
        pr = c.pairs[i]
        npairs = int(np.count_nonzero(pr[:, 1]))
        if npairs == 0:
            continue
        starts = [c.poses[i]]
        for ulps in PROBE_ULPS:
            up = dn = c.poses[i]
            for _ in range(ulps):
                up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            starts += [up, dn]
        runs = [orc.optimise_pose(c.markers, c.K, c.blobs, pr, s) for s in starts]
        pose[i], cov[i] = runs[0][0], runs[0][1]
        its = [r[2] for r in runs]
        cls[i] = OTHER
        if all(it >= rr.ORC_CAP for it in its):
            cls[i] = CAP_STABLE
            reverted[i] = all(r[0].tobytes() == np.ascontiguousarray(s).tobytes() for r, s in zip(runs, starts))
        elif all(it < rr.ORC_CAP for it in its):
            with np.errstate(invalid="ignore", over="ignore"):
                d = max(np.abs(a[0] - b[0]).max() for k, a in enumerate(runs) for b in runs[k + 1:])
            if d <= STABLE_TOL:  # (a NaN fails the comparison)
                cls[i] = STABLE
                if npairs >= 4:
                    top = np.abs(runs[0][1]).max()
                    spread = max(spread, float(np.abs(runs[1][1] - runs[0][1]).max() / top),
                                 float(np.abs(runs[2][1] - runs[0][1]).max() / top))  # (+-1 ulp, as rr.oracle_refine)
    return cls, pose, cov, reverted, spread


def same_or_close(got, want, rtol):
    if not (np.isfinite(got) and np.isfinite(want)):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= rtol * max(abs(want), 1e-300)


def untouched_by_the_iteration(c, rows):
    """n_pairs, rms_before, rms_after at the row's own pose, the status accounting: every row of every case.  Returns
    the largest relative rms difference over the finite ones."""
    p = gc.params(c)
    worst = 0.0
    for i in range(len(rows)):
        r, pr = rows[i], c.pairs[i]
        npairs = int(np.count_nonzero(pr[:, 1]))
        assert r["n_pairs"] == npairs and r["pad"] == 0, (c.name, i)
        if npairs == 0:
            assert r["status"] == pf.REFINE_NO_PAIRS and r["iters"] == 0, (c.name, i)
            assert r["rms_before"] == 0.0 and r["rms_after"] == 0.0, (c.name, i)
            assert r["pose"].tobytes() == np.ascontiguousarray(c.poses[i]).tobytes(), (c.name, i)
            continue
        with np.errstate(all="ignore"):
            before = rr.numpy_rms(c.markers, c.K, c.blobs, pr, c.poses[i])
            after = rr.numpy_rms(c.markers, c.K, c.blobs, pr, r["pose"])
        assert same_or_close(r["rms_before"], before, rr.RMS_RTOL), (c.name, i, r["rms_before"], before)
        assert same_or_close(r["rms_after"], after, rr.RMS_RTOL), (c.name, i, r["rms_after"], after)
        for got, want in ((r["rms_before"], before), (r["rms_after"], after)):
            if np.isfinite(got) and np.isfinite(want):
                worst = max(worst, abs(got - want) / max(abs(want), 1e-300))
        if r["status"] == pf.REFINE_CONVERGED:
            assert 0 <= r["iters"] < p.max_iter, (c.name, i)
        else:
            assert r["status"] in CAPS and r["iters"] == p.max_iter, (c.name, i, r["status"], r["iters"])
            if r["status"] == pf.REFINE_CAP_REVERTED:
                assert p.revert_on_divergence, (c.name, i)
                assert r["pose"].tobytes() == np.ascontiguousarray(c.poses[i]).tobytes(), (c.name, i)
    return worst


ORACLE_IDS = [cid for cid in gc.CASE_IDS if not cid.startswith("param-")]


@pytest.mark.parametrize("cid", ORACLE_IDS)
def test_host_against_oracle(cid):
    c = gc.case_by_id(cid)
    assert c.oracle
    rows, cov = gc.host_rows(c)
    cls, opose, ocov, orev, spread = classify(cid)
    drms = untouched_by_the_iteration(c, rows)
    with_pairs = int(np.count_nonzero(cls != NO_PAIRS))
    n_stable, n_cap = int(np.count_nonzero(cls == STABLE)), int(np.count_nonzero(cls == CAP_STABLE))
    dt = dr = dc = 0.0
    cov_bar = rr.COV_MARGIN * spread
    bad = []
    for i in np.flatnonzero(cls == STABLE):
        if rows["status"][i] != pf.REFINE_CONVERGED:
            bad.append((int(i), "stable, host status", int(rows["status"][i])))
            continue
        dt = max(dt, float(np.abs(rows["pose"][i][[3, 7, 11]] - opose[i][[3, 7, 11]]).max()))
        dr = max(dr, rr.rot_dist(rows["pose"][i], opose[i]))
        if rows["n_pairs"][i] >= 4:
            dc = max(dc, float(np.abs(cov[i] - ocov[i]).max() / np.abs(ocov[i]).max()))
    for i in np.flatnonzero(cls == CAP_STABLE):
        want = pf.REFINE_CAP_REVERTED if orev[i] else pf.REFINE_CAP_KEPT
        if rows["status"][i] != want or rows["iters"][i] != rr.ORC_CAP:
            bad.append((int(i), "cap-stable, host status / iters", int(rows["status"][i]), int(rows["iters"][i]), want))
    share_all = (n_stable + n_cap) / max(with_pairs, 1)
    full_rank = int(np.count_nonzero(rows["n_pairs"] >= rr.MIN_DETERMINED))
    few_ok = int(np.count_nonzero((rows["n_pairs"] > 0) & (rows["n_pairs"] < rr.MIN_DETERMINED) & (cls != OTHER)))
    share = (n_stable + n_cap - few_ok) / max(full_rank, 1)
    print(f"{cid}: {len(rows)} rows, {with_pairs} with pairs: {n_stable} stable, {n_cap} cap-stable "
          f"({int(np.count_nonzero(orev & (cls == CAP_STABLE)))} reverted), {with_pairs - n_stable - n_cap} other; share "
          f"{share:.3f} of the {full_rank} rows with 3 pairs or more ({share_all:.3f} of all with pairs), cap-stable share {n_cap / max(with_pairs, 1):.3f}; max dt {dt:.3e} m, dr {dr:.3e} rad, cov rel "
          f"{dc:.3e} (oracle's own spread {spread:.3e}, bar {cov_bar:.3e}), rms rel {drms:.3e}")
    assert not bad, (cid, bad[:8])
    assert dt <= rr.POSE_BAR and dr <= rr.POSE_BAR, (cid, dt, dr)
    assert dc <= cov_bar, (cid, dc, cov_bar)
    undetermined = c.group == "bucket" and len(c.markers) < 3
    if (c.group in ("bucket", "K", "scene1.7") and not undetermined) or cid == "ties":
        assert full_rank >= 100 and share >= 0.9, (cid, share, share_all)
    if undetermined:
        assert n_stable == 0, cid  # (what the module docstring says of them)
    if c.group == "scene0.5" and len(c.markers) in (4, 5):
        assert n_cap >= 0.25 * with_pairs, (cid, n_cap, with_pairs)


@pytest.mark.parametrize("cid", [cid for cid in gc.CASE_IDS if cid.startswith("param-")])
def test_host_parameters(cid):
    c = gc.case_by_id(cid)
    rows, cov = gc.host_rows(c)
    untouched_by_the_iteration(c, rows)
    p = gc.params(c)
    conv = rows["status"] == pf.REFINE_CONVERGED
    with_pairs = rows["n_pairs"] > 0
    print(f"{cid}: {int(with_pairs.sum())} rows with pairs: {int(conv.sum())} converged, "
          f"{int(np.count_nonzero(rows['status'] == pf.REFINE_CAP_KEPT))} kept, "
          f"{int(np.count_nonzero(rows['status'] == pf.REFINE_CAP_REVERTED))} reverted, iters max {int(rows['iters'].max())}")
    assert with_pairs.sum() >= 20
    if not p.revert_on_divergence:
        assert not np.any(rows["status"] == pf.REFINE_CAP_REVERTED)
    # against the same rows under the defaults: a row that converges there within this case's max_iter, under a
    # threshold no looser than this case's, converges here at the same iteration with the same bytes
    base = gc.scene_case(0.5, len(c.markers))
    brows, bcov = gc.host_rows(base)
    brows, bcov = brows[c.note["sel"]], bcov[c.note["sel"]]
    n = len(rows)
    if p.converged == 1e-13:
        same = (brows["status"][:n] == pf.REFINE_CONVERGED) & (brows["iters"][:n] < p.max_iter)
        assert rows[same].tobytes() == brows[:n][same].tobytes() and cov[same].tobytes() == bcov[:n][same].tobytes()
        assert not np.any(conv & with_pairs & ~same), cid
    elif p.converged > 1e-13:  # a looser threshold stops no later
        assert np.all(rows["iters"][with_pairs] <= np.minimum(brows["iters"][:n][with_pairs], p.max_iter))
    else:  # converged = 0: only a step of exactly zero ends the iteration
        assert np.all(rows["iters"][with_pairs] >= np.minimum(brows["iters"][:n][with_pairs], p.max_iter))
    if "keep" in cid:  # the divergence rule off: the rows that reverted under it are kept, the others are the same bytes
        on = dict(c.prm)
        on.pop("revert_on_divergence")
        twin = gc.Case(c.name + "-on", c.markers, c.K, c.blobs, c.poses, c.pairs, prm=on, oracle=False)
        trows, tcov = gc.host_rows(twin)
        rev = trows["status"] == pf.REFINE_CAP_REVERTED
        assert np.all(rows["status"][rev] == pf.REFINE_CAP_KEPT)
        assert rows[~rev].tobytes() == trows[~rev].tobytes() and cov[~rev].tobytes() == tcov[~rev].tobytes()
        print(f"{cid}: {int(rev.sum())} rows revert with the rule on")
        if p.max_iter == 3:
            assert rev.sum() >= 1


# ------------------------------------------------------------------------------------------------ far starts
def quarter(th):
    return int(np.floor(th * 6.36619772367581382433e-01 + 0.5)) & 3


def test_far_starts_do_what_they_are_for():
    """From numpy's own solve of the first normal equations: over the 5-LED set the first step's |omega| reaches all
    four quarter-turn cases of gn_sincos; and the 12-LED set leaves rows at the cap on the host, kept and reverted."""
    c = gc.far_case(5)
    th = np.array([np.linalg.norm(gc.first_step(c, i)[3:]) for i in range(len(c.poses))])
    seen = {quarter(t) for t in th}
    print(f"far-M5: first-step |omega| from {th.min():.3f} to {th.max():.3f} rad, quarter-turn cases {sorted(seen)}")
    assert seen == {0, 1, 2, 3}
    rows, _ = gc.host_rows(gc.far_case(12))
    kept = int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_KEPT))
    rev = int(np.count_nonzero(rows["status"] == pf.REFINE_CAP_REVERTED))
    print(f"far-M12: {kept} rows kept at the cap, {rev} reverted, {int(np.count_nonzero(rows['status'] == pf.REFINE_CONVERGED))} converged")
    assert kept >= 1 and rev >= 1


# ------------------------------------------------------------------------------------------ literal assertions
def test_degenerate_rows():
    c = gc.degenerate_case()
    rows, cov = gc.host_rows(c)
    for kind in ("on_axis", "z0", "behind", "nan_x", "inf_y", "two_leds_one_blob", "led_twice", "all16", "holes", "no_pairs"):
        assert len(c.note[kind]) >= 3, kind
    # one pair, its LED on the optical axis: two diagonals of A are exactly 0, the factorisation reports the zero pivot,
    # the step is 0: CONVERGED at once with the input pose's bytes and an all-zero covariance; the oracle agrees
    for i in c.note["on_axis"]:
        r = rows[i]
        assert r["status"] == pf.REFINE_CONVERGED and r["iters"] == 0 and r["n_pairs"] == 1, i
        assert r["pose"].tobytes() == np.ascontiguousarray(c.poses[i]).tobytes(), i
        assert not cov[i].any() and r["rms_after"] == r["rms_before"], i
        po, co, it = orc.optimise_pose(c.markers, c.K, c.blobs, c.pairs[i], c.poses[i])
        assert it == 0 and po.tobytes() == np.ascontiguousarray(c.poses[i]).tobytes(), i
    # a paired LED in the camera's plane: the projection divides by 0
    for i in c.note["z0"]:
        assert np.all(np.isnan(rows["pose"][i])) and np.isnan(rows["rms_after"][i]), i
    for kind in ("nan_x", "inf_y"):
        for i in c.note[kind]:
            assert not np.isfinite(rows["rms_after"][i]) and not np.isfinite(rows["rms_before"][i]), (kind, i)
    best = gc.best_of(rows)
    not_eligible = set(c.note["z0"]) | set(c.note["nan_x"]) | set(c.note["inf_y"]) | set(c.note["no_pairs"])
    assert best >= 0 and best not in not_eligible
    assert rows["n_pairs"][best] == 16 and best in set(c.note["all16"])
    for i in c.note["all16"]:
        assert rows["status"][i] == pf.REFINE_CONVERGED and rows["rms_after"][i] < 1e-6, i
    # rows with holes: as the same pairs without them
    for i in c.note["holes"]:
        used = c.pairs[i][c.pairs[i][:, 1] != 0]
        r, cv = pf.host_optimise_pose(c.markers, c.K, c.blobs, used, c.poses[i])
        assert r.tobytes() == rows[i].tobytes() and cv.tobytes() == cov[i].tobytes(), i
    # no pairs: as test_refine_host.py::test_no_pairs_returns_the_input has it
    for i in c.note["no_pairs"]:
        r = rows[i]
        assert r["status"] == pf.REFINE_NO_PAIRS and r["n_pairs"] == 0 and r["iters"] == 0, i
        assert r["pose"].tobytes() == np.ascontiguousarray(c.poses[i]).tobytes(), i
        assert r["rms_before"] == 0.0 and r["rms_after"] == 0.0 and not cov[i].any(), i


def test_ties_are_ties():
    c = gc.tie_case()
    rows, _ = gc.host_rows(c)
    copies = c.note["copies"]
    assert len(copies) >= len(gc.TIE_AT)
    assert all(rows[i].tobytes() == rows[copies[0]].tobytes() for i in copies)
    assert gc.best_of(rows) == c.note["best"] == copies[0]
