"""Host side of the Gauss-Newton refinement (pfmpe_refine_poses / pfmpe_refine_cloud / pfmpe_host_optimise_pose): the
symbols, layouts and defaults, pfmpe_host_optimise_pose (the code a lane of k_refine runs) against the oracle's
optimisePose on the three test clouds under the rules of refine_ref.py, and its edge cases.  No GPU."""
import ctypes

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi

import refine_ref as rr


def test_symbols_listed_and_exported():
    lib = pf.load()
    for name in ("pfmpe_default_refine_params", "pfmpe_refine_poses", "pfmpe_refine_cloud", "pfmpe_host_optimise_pose"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert (pf.REFINE_NO_PAIRS, pf.REFINE_CONVERGED, pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED) == (0, 1, 2, 3)


def test_struct_sizes_and_defaults():
    assert ctypes.sizeof(_capi.RefineRow) == 128
    assert pf.REFINE_ROW_DTYPE.itemsize == 128
    assert ctypes.sizeof(_capi.RefineParams) == 16
    assert ctypes.sizeof(_capi.RefineOut) == 6 * 8 + 8 + 8 + 128 + 36 * 8
    p = pf.default_refine_params()
    assert (p.max_iter, p.revert_on_divergence, p.converged) == (500, 1, 1e-13)


def host_rows(markers, K, blobs, poses, pairs, params=None):
    rows = np.zeros(len(poses), dtype=pf.REFINE_ROW_DTYPE)
    cov = np.zeros((len(poses), 6, 6))
    for i in range(len(poses)):
        rows[i], cov[i] = pf.host_optimise_pose(markers, K, blobs, pairs[i], poses[i], params)
    return rows, cov


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_against_oracle(name):
    markers, K, blobs, poses, pairs, ref = rr.cloud(name)
    rows, cov = host_rows(markers, K, blobs, poses, pairs)
    print(f"{name}: oracle under +-1 ulp: cov spread {ref['cov_spread']:.3e}, pose spread {ref['pose_spread_determined']:.3e} m "
          f"(>= 3 pairs) / {ref['pose_spread_undetermined']:.3e} m (1-2 pairs)")
    rr.compare(f"host {name}", rows, cov, ref, ref["iters"] < rr.ORC_CAP, markers, K, blobs, poses, pairs,
               rr.COV_MARGIN * ref["cov_spread"])
    conv = rows["status"] == pf.REFINE_CONVERGED
    assert np.all(rows["iters"][conv] < 500) and np.all(rows["iters"][~conv & (rows["n_pairs"] > 0)] == 500)


def _one(name="A", i=None):
    markers, K, blobs, poses, pairs, ref = rr.cloud(name)
    if i is None:
        i = int(np.flatnonzero(ref["n_pairs"] == rr.CONFIGS[name][0])[0])  # a row with every LED paired
    return markers, K, blobs, poses[i].copy(), pairs[i].copy(), ref, i


def test_no_pairs_returns_the_input():
    markers, K, blobs, pose, pairs, _, _ = _one()
    for pr in (np.zeros((0, 2), dtype=np.uint32), np.array([[1, 0], [3, 0], [0, 0]], dtype=np.uint32)):
        row, cov = pf.host_optimise_pose(markers, K, blobs, pr, pose)
        assert row["status"] == pf.REFINE_NO_PAIRS and row["n_pairs"] == 0 and row["iters"] == 0
        assert row["pose"].tobytes() == pose.tobytes()
        assert row["rms_before"] == 0.0 and row["rms_after"] == 0.0
        assert not cov.any()


def test_zero_row_in_the_middle_is_skipped():
    markers, K, blobs, pose, pairs, _, _ = _one()
    used = pairs[pairs[:, 1] != 0]
    holed = np.concatenate([used[:2], np.zeros((1, 2), dtype=np.uint32), used[2:]])
    a, ca = pf.host_optimise_pose(markers, K, blobs, used, pose)
    b, cb = pf.host_optimise_pose(markers, K, blobs, holed, pose)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    assert a["n_pairs"] == len(used) and a["status"] == pf.REFINE_CONVERGED


def test_one_pair_is_finite():
    markers, K, blobs, pose, pairs, _, _ = _one()
    row, cov = pf.host_optimise_pose(markers, K, blobs, pairs[:1], pose)
    assert row["n_pairs"] == 1
    assert np.all(np.isfinite(row["pose"])) and np.isfinite(row["rms_before"]) and np.isfinite(row["rms_after"])
    assert np.all(np.isfinite(cov))


def test_max_iter_one_is_a_cap():
    markers, K, blobs, pose, pairs, _, _ = _one()
    p = pf.default_refine_params()
    p.max_iter = 1
    row, _ = pf.host_optimise_pose(markers, K, blobs, pairs, pose, p)
    assert row["iters"] == 1 and row["status"] in (pf.REFINE_CAP_KEPT, pf.REFINE_CAP_REVERTED)


def test_no_revert_never_reports_reverted():
    # few iterations, so many rows stop at the cap; with the rule on, some of them revert to the start pose
    markers, K, blobs, poses, pairs, ref = rr.cloud("A")
    sel = np.flatnonzero(ref["n_pairs"] > 0)[:200]
    p = pf.default_refine_params()
    p.max_iter = 3
    on, _ = host_rows(markers, K, blobs, poses[sel], pairs[sel], p)
    p.revert_on_divergence = 0
    off, _ = host_rows(markers, K, blobs, poses[sel], pairs[sel], p)
    assert not np.any(off["status"] == pf.REFINE_CAP_REVERTED)
    rev = on["status"] == pf.REFINE_CAP_REVERTED
    for i in np.flatnonzero(rev):
        assert on["pose"][i].tobytes() == poses[sel][i].tobytes()
        assert off["status"][i] == pf.REFINE_CAP_KEPT
    same = ~rev
    assert on[same].tobytes() == off[same].tobytes()


def test_bad_arguments():
    markers, K, blobs, pose, pairs, _, _ = _one()
    used = pairs[pairs[:, 1] != 0]

    def code(pr=used, ps=pose, **kw):
        p = pf.default_refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(pf.PFError) as e:
            pf.host_optimise_pose(markers, K, blobs, pr, ps, p)
        return e.value.code

    bad = used.copy()
    bad[0, 0] = len(markers) + 1
    assert code(pr=bad) == pf.E_ARG
    bad = used.copy()
    bad[0, 1] = len(blobs) + 1
    assert code(pr=bad) == pf.E_ARG
    bad = used.copy()
    bad[0, 0] = 0
    assert code(pr=bad) == pf.E_ARG
    for v in (0, -1, 10001):
        assert code(max_iter=v) == pf.E_ARG
    assert code(converged=-1e-13) == pf.E_ARG
    assert code(converged=float("nan")) == pf.E_ARG
    nanpose = pose.copy()
    nanpose[5] = np.inf
    assert code(ps=nanpose) == pf.E_ARG
    # the limits themselves are fine
    for kw in ({"max_iter": 1}, {"max_iter": 10000}, {"converged": 0.0}):
        p = pf.default_refine_params()
        for k, v in kw.items():
            setattr(p, k, v)
        pf.host_optimise_pose(markers, K, blobs, used, pose, p)
    lib = pf.load()
    row = _capi.RefineRow()
    assert lib.pfmpe_host_optimise_pose(None, 5, None, None, 0, None, 0, None, None, ctypes.byref(row), None) == pf.E_ARG
