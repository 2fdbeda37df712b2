"""Host side of the association statistics (pfmpe_assoc_stats / pfmpe_get_pairs / pfmpe_host_assoc_summary): the
struct layouts, the exported symbols and the summary of hand-made votes tables.  No GPU."""
import ctypes

import numpy as np
import pytest

import pf_monocular_pose_estimator_amd as pf
from pf_monocular_pose_estimator_amd import _capi


def test_struct_sizes():
    assert ctypes.sizeof(_capi.AssocOut) == 352
    assert ctypes.sizeof(_capi.AssocIn) == 16


def test_symbols_listed_and_exported():
    lib = pf.load()
    for name in ("pfmpe_assoc_stats", "pfmpe_get_pairs", "pfmpe_host_assoc_summary"):
        assert name in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert (pf.ASSOC_PROPAGATED, pf.ASSOC_POSTERIOR) == (0, 1)


def _table(rows):
    return np.array(rows, dtype=np.uint32)


def test_clear_mode():
    # 10 particles, 2 LEDs, 3 blobs; column 0 = unpaired
    got = pf.host_assoc_summary(_table([[1, 0, 7, 2], [0, 9, 0, 1]]))
    assert (got["n"], got["M"], got["B"]) == (10, 2, 3)
    assert got["matched"].tolist() == [9, 10]
    assert got["mode_blob"].tolist() == [2, 1]
    assert got["mode_votes"].tolist() == [7, 9]
    assert got["second_votes"].tolist() == [2, 1]
    assert set(got) == {"n", "M", "B", "matched", "mode_blob", "mode_votes", "second_votes"}


def test_tie_takes_lowest_blob():
    got = pf.host_assoc_summary(_table([[2, 1, 4, 0, 4, 1], [0, 6, 6, 0, 0, 0]]))
    assert got["mode_blob"].tolist() == [2, 1]
    assert got["mode_votes"].tolist() == [4, 6]
    assert got["second_votes"].tolist() == [4, 6]
    assert got["n"] == 12 and got["matched"].tolist() == [10, 12]


def test_unmatched_led():
    got = pf.host_assoc_summary(_table([[5, 0, 0], [1, 4, 0]]))
    assert got["n"] == 5
    assert got["mode_blob"].tolist() == [0, 1]
    assert got["matched"].tolist() == [0, 4]
    assert got["mode_votes"].tolist() == [0, 4]
    assert got["second_votes"].tolist() == [0, 0]


def test_no_blobs():
    got = pf.host_assoc_summary(_table([[7], [7], [7]]))
    assert (got["n"], got["M"], got["B"]) == (7, 3, 0)
    for k in ("matched", "mode_blob", "mode_votes", "second_votes"):
        assert got[k].tolist() == [0, 0, 0]


def test_unequal_rows_refused():
    with pytest.raises(pf.PFError) as e:
        pf.host_assoc_summary(_table([[1, 2, 3], [1, 2, 4]]))
    assert e.value.code == pf.E_ARG


def test_raw_arguments():
    lib = pf.load()
    v = _table([[1, 2]])
    vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    out = _capi.AssocOut()
    assert lib.pfmpe_host_assoc_summary(vp, 1, 1, ctypes.byref(out)) == pf.OK
    assert (out.n, out.n_any, out.matched[0], out.mode_blob[0]) == (3, 0, 2, 1)
    assert lib.pfmpe_host_assoc_summary(None, 1, 1, ctypes.byref(out)) == pf.E_ARG
    assert lib.pfmpe_host_assoc_summary(vp, 1, 1, None) == pf.E_ARG
    assert lib.pfmpe_host_assoc_summary(vp, 0, 1, ctypes.byref(out)) == pf.E_ARG
    assert lib.pfmpe_host_assoc_summary(vp, pf.MAX_MARKERS + 1, 1, ctypes.byref(out)) == pf.E_ARG
    assert lib.pfmpe_host_assoc_summary(vp, 1, -1, ctypes.byref(out)) == pf.E_ARG


def test_as_dict_trims_to_m():
    out = _capi.AssocOut()
    out.M, out.B, out.n = 3, 4, 9
    d = out.as_dict()
    assert all(len(d[k]) == 3 for k in ("matched", "mode_blob", "mode_votes", "second_votes"))
    assert len(d["npairs_hist"]) == 4
