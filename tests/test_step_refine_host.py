"""pfmpe_host_step_tail (no GPU): the code the step's tail runs on a finished frame, on the host.

For an accepted frame with a finite winner pose it is Gauss-Newton of the winner over the frame's pair row, so it must
give pfmpe_host_optimise_pose's row and covariance byte for byte (the same __host__ __device__ function on the same
numbers; the tail only gathers the blobs the row names into a compact list first) and pfmpe_refine_poses' summary of
one hypothesis.  A frame that is not refined gives the K = 0 summary and leaves the caller's row and covariance alone.
"""
import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import synthetic as syn

import refine_ref as rr

N_HYP = 24


def frame_of(pose, pairs, flag=pf.FLAG_ACCEPTED):
    fo = pf.FrameOut()
    fo.flag_fail = flag
    fo.accepted = 1 if flag == pf.FLAG_ACCEPTED else 0
    fo.winner_pose[:] = list(np.asarray(pose, np.float64).reshape(12))
    pr = np.asarray(pairs, np.uint32).reshape(-1)
    fo.corr[: len(pr)] = list(pr)
    fo.n_corr = int(np.count_nonzero(pr.reshape(-1, 2)[:, 1]))
    return fo


def hypotheses(name):
    markers, K, blobs, T = rr.scene(name)
    poses = syn.initial_prior(T, N_HYP)
    return markers, K, blobs, poses, rr.oracle_pairs(markers, K, blobs, poses)


def summary_of(row):
    """pfmpe_refine_poses' summary of the one hypothesis whose row this is."""
    ok = row.n_pairs > 0 and np.isfinite(row.rms_after)
    return dict(n=1, n_with_pairs=int(row.n_pairs > 0), n_converged=int(row.status == pf.REFINE_CONVERGED),
                n_cap_kept=int(row.status == pf.REFINE_CAP_KEPT), n_cap_reverted=int(row.status == pf.REFINE_CAP_REVERTED),
                iters_total=row.iters, iters_max=row.iters, best=0 if ok else -1)


def assert_empty(gn):
    assert gn.n == 0 and gn.best == -1
    assert not np.frombuffer(bytes(gn), dtype=np.uint8)[:56].any()  # the counts
    assert not np.frombuffer(bytes(gn.best_row), dtype=np.uint8).any() and not np.array(gn.best_cov).any()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_accepted_frames_equal_host_optimise_pose(name):
    markers, K, blobs, poses, pairs = hypotheses(name)
    with_pairs = 0
    for i in range(N_HYP):
        ref = pf.host_optimise_pose(markers, K, blobs, pairs[i], poses[i])
        rrow, rcov = ref[0], ref[1]
        gn, row, cov = pf.host_step_tail(markers, K, blobs, frame_of(poses[i], pairs[i]))
        assert bytes(row) == rrow.tobytes(), i
        assert cov.tobytes() == np.ascontiguousarray(rcov, dtype=np.float64).tobytes(), i
        want = summary_of(row)
        for k, v in want.items():
            assert getattr(gn, k) == v, (i, k)
        if want["best"] == 0:
            assert bytes(gn.best_row) == bytes(row) and np.array(gn.best_cov).tobytes() == cov.tobytes(), i
        else:
            assert not np.frombuffer(bytes(gn.best_row), dtype=np.uint8).any() and not np.array(gn.best_cov).any(), i
        with_pairs += row.n_pairs > 0
    # the clouds have work for Gauss-Newton: about a quarter of the rows of A and B have pairs (refine_ref.py: 547 and
    # 533 of 2,048), nearly all of C
    assert with_pairs >= 3


def test_refine_params_reach_the_tail():
    markers, K, blobs, poses, pairs = hypotheses("A")
    i = int(np.flatnonzero(np.count_nonzero(pairs[:, :, 1], axis=1) >= 3)[0])
    for revert in (1, 0):
        prm = pf.default_refine_params()
        prm.max_iter, prm.revert_on_divergence = 1, revert
        ref = pf.host_optimise_pose(markers, K, blobs, pairs[i], poses[i], params=prm)
        gn, row, cov = pf.host_step_tail(markers, K, blobs, frame_of(poses[i], pairs[i]), params=prm)
        assert bytes(row) == ref[0].tobytes()
        assert row.iters == 1 and row.status in (pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED)
        assert gn.n_cap_kept + gn.n_cap_reverted == 1 and gn.n_converged == 0


@pytest.mark.parametrize("case", ["reinit", "nan"])
def test_frames_that_are_not_refined(case):
    markers, K, blobs, poses, pairs = hypotheses("A")
    fo = frame_of(poses[0], pairs[0], flag=pf.FLAG_REINIT if case == "reinit" else pf.FLAG_ACCEPTED)
    if case == "nan":
        fo.winner_pose[7] = float("nan")
    row = pf.RefineRow()
    row.pose[:] = [-3.5] * 12
    row.iters, row.n_pairs, row.status = 77, 66, 55
    before = bytes(row)
    cov = np.full(36, -7.25)
    gn, row2, cov2 = pf.host_step_tail(markers, K, blobs, fo, row=row, cov=cov)
    assert_empty(gn)
    assert bytes(row) == before and (cov == -7.25).all()


def test_rows_with_blob_zero_are_skipped():
    markers, K, blobs, poses, pairs = hypotheses("A")
    i = int(np.flatnonzero(np.count_nonzero(pairs[:, :, 1], axis=1) >= 4)[0])
    pr = pairs[i].copy()
    used = np.flatnonzero(pr[:, 1])
    pr[used[1], 1] = 0  # an LED that found no blob, in the middle of the row
    ref = pf.host_optimise_pose(markers, K, blobs, pr, poses[i])
    gn, row, cov = pf.host_step_tail(markers, K, blobs, frame_of(poses[i], pr))
    assert row.n_pairs == len(used) - 1
    assert bytes(row) == ref[0].tobytes()
    assert cov.tobytes() == np.ascontiguousarray(ref[1], dtype=np.float64).tobytes()
    # a frame without any pair: the start pose comes back, NO_PAIRS, and no best hypothesis
    gn, row, cov = pf.host_step_tail(markers, K, blobs, frame_of(poses[i], np.zeros((pf.MAX_MARKERS, 2))))
    assert row.status == pf.REFINE_NO_PAIRS and row.n_pairs == 0 and gn.n == 1 and gn.best == -1
    assert np.array(row.pose).tobytes() == np.ascontiguousarray(poses[i]).tobytes()


@pytest.mark.parametrize("bad", ["max_iter0", "max_iter_big", "neg_converged", "nan_converged"])
def test_bad_parameters(bad):
    markers, K, blobs, poses, pairs = hypotheses("A")
    prm = pf.default_refine_params()
    if bad == "max_iter0":
        prm.max_iter = 0
    elif bad == "max_iter_big":
        prm.max_iter = 10001
    elif bad == "neg_converged":
        prm.converged = -1e-9
    else:
        prm.converged = float("nan")
    with pytest.raises(pf.PFError) as e:
        pf.host_step_tail(markers, K, blobs, frame_of(poses[0], pairs[0]), params=prm)
    assert e.value.code == pf.E_ARG


def test_bad_indices_and_arguments():
    markers, K, blobs, poses, pairs = hypotheses("A")
    pr = pairs[0].copy()
    pr[0] = (1, len(blobs) + 1)  # a blob the list does not have
    with pytest.raises(pf.PFError):
        pf.host_step_tail(markers, K, blobs, frame_of(poses[0], pr))
    pr[0] = (len(markers) + 1, 1)  # an LED the model does not have
    with pytest.raises(pf.PFError):
        pf.host_step_tail(markers, K, blobs, frame_of(poses[0], pr))
    # ... which a frame that is not refined never looks at
    gn, _, _ = pf.host_step_tail(markers, K, blobs, frame_of(poses[0], pr, flag=pf.FLAG_REINIT))
    assert_empty(gn)
