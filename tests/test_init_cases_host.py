"""The envelope cases of tests/init_cases.py are what their names say: checked on the CPU with the oracle, so that the
GPU tests of tests/test_gpu_init_envelope.py cannot pass by comparing two runs of something else.  No GPU."""
import dataclasses
import math

import numpy as np
import pytest

import init_cases as ic
from oracle import pforacle as orc

HIST = {c.name: c for c in ic.histogram_cases()}
INIT = {c.name: c for c in ic.initialise_cases()}
THRESH = 10000.0 * 100.0  # threshDist = threshDist2, px^2 (PE:1557-1558)


def run_oracle(c, N=None, **kw):
    return orc.initialise(c.markers, c.K, c.blobs, N or c.N, tol=c.tol, certainty_threshold=c.certainty_threshold,
                          valid_corr_threshold=c.valid_corr_threshold, max_candidates=c.max_candidates, **kw)


def test_case_list_covers_what_it_should():
    assert {c.M for c in HIST.values()} >= {4, 13, 16}
    assert {c.tol for c in HIST.values()} >= {1.0, 5.0, 12.0}
    assert HIST["M4_B4"].M == HIST["M4_B4"].B == 4
    k = HIST["other_camera"].K
    assert k[0, 0] != k[1, 1] and not np.array_equal(k, ic.syn.K_README)


@pytest.mark.parametrize("name", sorted(HIST))
def test_histogram_case_is_small_and_not_trivial(name):
    c = HIST[name]
    assert c.B >= 3 and 3 <= c.M <= 16
    assert math.comb(c.B, 3) * c.M * (c.M - 1) * (c.M - 2) <= 1_000_000
    h, lo, hi, _ = orc.init_histogram_bounds(c.markers, c.K, c.blobs, tol=c.tol)
    assert np.array_equal(h, orc.init_histogram(c.markers, c.K, c.blobs, tol=c.tol))
    assert (h.sum() == 0) == c.empty
    assert (lo <= h).all() and (h <= hi).all()


def sqd(a, b):
    return (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2


def test_blob_geometry_cases():
    b = HIST["equal_x"].blobs
    assert b[6, 0] == b[1, 0] and b[6, 1] != b[1, 1]
    b = HIST["identical_blobs"].blobs
    assert np.array_equal(b[-1], b[2])
    b = HIST["outside_image"].blobs
    assert (b < 0).any() and (b[:, 0] > ic.syn.IMAGE_W).any() and (b[:, 1] > ic.syn.IMAGE_H).any()


def test_pair_at_1000px_decides_the_histogram():
    """The pair at exactly 1000 px belongs to scoring combinations: one ulp farther, where "> threshDist" holds, they
    are gone and the histogram is another one; one ulp nearer it is the same.  So a filter with ">=" for ">", on
    either case, gives a histogram outside the band."""
    at, beyond = HIST["pair_1000px"], HIST["pair_beyond_1000px"]
    assert sqd(at.blobs[0], at.blobs[1]) == THRESH  # exactly 1000 px: not "> threshDist"
    assert THRESH < sqd(beyond.blobs[0], beyond.blobs[1]) < THRESH * (1 + 1e-12)
    assert np.array_equal(at.blobs[[0, 2, 3, 4, 5, 6]], beyond.blobs[[0, 2, 3, 4, 5, 6]])
    h_at, lo_at, hi_at, _ = orc.init_histogram_bounds(at.markers, at.K, at.blobs, tol=at.tol)
    h_be, lo_be, hi_be, _ = orc.init_histogram_bounds(beyond.markers, beyond.K, beyond.blobs, tol=beyond.tol)
    assert h_at[1].sum() > 0  # the blob placed at 1000 px scores
    nearer = at.blobs.copy()
    nearer[1, 0] = np.nextafter(nearer[1, 0], -np.inf)
    assert np.array_equal(orc.init_histogram(at.markers, at.K, nearer, tol=at.tol), h_at)
    # each case's histogram lies outside the other's band, beyond the allowance of the GPU test
    for h, lo, hi, other in ((h_at, lo_at, hi_at, h_be), (h_be, lo_be, hi_be, h_at)):
        h, lo, hi, other = (x.astype(np.int64) for x in (h, lo, hi, other))
        assert ((other < lo) | (other > hi)).any()
        assert np.abs(other - h).sum() > max(4, 0.005 * h.sum())


def test_centroid_count_cases():
    # the centroid's count over the combinations whose pairs are all in range
    for name, want in (("centroid_5", 5), ("centroid_4", 4)):
        b = HIST[name].blobs
        counts = set()
        for i in range(len(b)):
            for j in range(i):
                for k in range(j):
                    if max(sqd(b[i], b[j]), sqd(b[i], b[k]), sqd(b[j], b[k])) > THRESH:
                        continue
                    m = (b[i] + b[j] + b[k]) / 3
                    counts.add(sum(1 for q in b if sqd(m, q) < THRESH))
        assert counts == {want}, (name, counts)


def test_collinear_model_has_a_collinear_triple():
    mk = ic.MARKERS_COLLINEAR
    assert np.linalg.norm(np.cross(mk[1] - mk[0], mk[2] - mk[0])) == 0.0
    fv = orc.image_vectors(ic.syn.K_README, HIST["collinear_model"].blobs[:3])
    assert orc.p3p(fv, mk[:3])[0] == -1


def test_initialise_cases_reach_their_flags():
    """With the oracle's own histogram: flag_fail 0, 6, 7, 8, 11 and 12, and the candidate cap, each at least once."""
    seen = set()
    for name, c in INIT.items():
        out, _, _ = run_oracle(c)
        if name in ic.EXPECTED_FLAGS:
            assert out["flag_fail"] == ic.EXPECTED_FLAGS[name], (name, out)
        assert out["found"] == (1 if out["flag_fail"] == 0 else 0)
        seen.add(out["flag_fail"])
    assert seen >= {0, 6, 7, 8, 11, 12}
    with pytest.raises(RuntimeError):
        run_oracle(ic.cap_case())
    c = ic.cap_case()
    c.max_candidates = 1 << 20
    run_oracle(c)  # the same blobs under the default cap: no error (the cap counts vectors before checkAmbiguity)


def test_valid_threshold_straddles():
    """valid_0.9 and valid_1.0 are one frame with 9 of 10 subsets valid: found at 0.9, flag 8 at 1.0; valid_0.9_below
    has 8 of 10: found at the default 0.5, flag 8 at 0.9."""
    a, b, c = INIT["valid_0.9"], INIT["valid_1.0"], INIT["valid_0.9_below"]
    assert np.array_equal(a.blobs, b.blobs) and a.tol == b.tol
    oa, ob, oc = run_oracle(a)[0], run_oracle(b)[0], run_oracle(c)[0]
    assert (oa["found"], oa["n_estimates"]) == (1, 9) and ob["flag_fail"] == 8 and ob["n_estimates"] == 9
    assert oc["flag_fail"] == 8 and oc["n_estimates"] == 8
    assert run_oracle(dataclasses.replace(c, valid_corr_threshold=0.5))[0]["found"] == 1


def test_certainty_and_valid_cases_differ_from_the_defaults():
    """The thresholds matter in their cases: another outcome than with the defaults."""
    for name in ("certainty_half_M6", "certainty_half_M7", "flag7", "flag8", "valid_1.0", "valid_0.9_below"):
        c = INIT[name]
        out, _, _ = run_oracle(c)
        ref, _, _ = orc.initialise(c.markers, c.K, c.blobs, c.N, tol=c.tol)
        assert (out["flag_fail"], out["n_estimates"], out["n_candidates"]) != \
            (ref["flag_fail"], ref["n_estimates"], ref["n_candidates"]), name


def test_particle_count_boundary():
    c = ic.boundary_case()
    K = run_oracle(c)[0]["n_estimates"]
    assert K >= 5  # N = M = 5 is below the number of valid subsets
    for N, found in ((5, 0), (K + 1, 0), (K + 2, 1)):
        out, _, _ = run_oracle(c, N=N)
        assert out["found"] == found, (N, out)
