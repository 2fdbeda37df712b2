"""The brute-force P3P (re)initialisation over its envelope (the cases of tests/init_cases.py, which
tests/test_init_cases_host.py shows on the CPU to be what their names say), through the C-ABI against the oracle.

Histogram cases: p3p_histogram against orc.init_histogram_bounds with the three band assertions of
tests/test_gpu_init.py::test_histogram_matches_oracle, unchanged; a case whose histogram is zero in the oracle
(no combination passes the spread filter) must be zero on the device too.

initialise cases: the oracle is fed the GPU's histogram; found, flag, candidate count, first match, stored-pose
count, histogram total and `pairs` are equal; predicted_pose within 1e-9 and the seeded set within the state's
storage precision (f64 1e-12, f32 4e-7, f16 1e-3), the bars of tests/test_gpu_init.py.

Measured on an MI355X (each test prints its figures before it asserts).  No case needed another bar than those:
predicted_pose differs by 2.3e-16 at most; the seeded set by 7.7e-16 (f64), 1.2e-7 (f32), 8.3e-4 (f16).  The device
reaches the flag of every case's name (0, 6, 7, 8, 11, 12) with its own histogram, the three valid_* cases on either
side of their threshold among them; the two pair_*1000px histograms (sums 74 and 55) are the oracle's exactly.
Histograms: equal to the oracle's in all cases but M13 (464 of 1,660,873 counts differ, 0.03 %), M16 (612 of 2,974,941, 0.02 %), tol12 (4 of 1,273) and
the collinear model (4 of 405, the floor of the allowance), all inside the band.
"""
import numpy as np
import pytest

import init_cases as ic
import pf_monocular_pose_estimator_amd as pf
from oracle import pforacle as orc

pytestmark = pytest.mark.gpu

HIST = ic.histogram_cases()
INIT = ic.initialise_cases()
STATES = {"f64": (pf.STATE_F64, 1e-12), "f32": (pf.STATE_F32, 4e-7), "f16": (pf.STATE_F16, 1e-3)}
DISCRETE = ("found", "flag_fail", "n_estimates", "n_candidates", "first_match", "hist_total")


def engine(c, N=None, state=pf.STATE_F64):
    eng = pf.Engine(device=0, max_particles=max(N or c.N, 16), state_dtype=state)
    eng.set_model(c.markers, c.K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_REFERENCE
    prm.tol = c.tol
    eng.set_params(prm)
    return eng


def gpu_initialise(eng, c, N=None):
    return eng.initialise(c.blobs, n_particles=N or c.N, certainty_threshold=c.certainty_threshold,
                          valid_corr_threshold=c.valid_corr_threshold, max_candidates=c.max_candidates)


def oracle_initialise(c, h, N=None, particles=None):
    return orc.initialise(c.markers, c.K, c.blobs, N or c.N, particles=particles, tol=c.tol,
                          certainty_threshold=c.certainty_threshold, valid_corr_threshold=c.valid_corr_threshold,
                          max_candidates=c.max_candidates, hist=h)


def assert_same_outcome(out, ref):
    for k in DISCRETE:
        assert out[k] == ref[k], (k, out[k], ref[k])
    assert np.array_equal(out["pairs"], ref["pairs"])


@pytest.fixture(scope="module")
def oracle_bounds():
    """The oracle's histogram and band of every histogram case, computed once."""
    return {c.name: orc.init_histogram_bounds(c.markers, c.K, c.blobs, tol=c.tol) for c in HIST}


@pytest.mark.parametrize("c", HIST, ids=lambda c: c.name)
def test_histogram_case_matches_oracle(c, oracle_bounds):
    eng = engine(c)
    h_gpu = eng.p3p_histogram(c.blobs).astype(np.int64)
    eng.close()
    h_ref, lo, hi, unbounded = oracle_bounds[c.name]
    h_ref, lo, hi = h_ref.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)
    print(f"{c.name}: sum {h_ref.sum()}, |gpu - oracle| {np.abs(h_gpu - h_ref).sum()}, band {int((hi - lo).sum())}")
    if c.empty:
        assert h_ref.sum() == 0 and h_gpu.sum() == 0
        return
    assert h_gpu.sum() > 0
    assert (h_gpu >= lo).all(), np.argwhere(h_gpu < lo)[:10]
    excess = np.maximum(h_gpu - hi, 0).sum()
    assert excess <= unbounded * (3 + c.M), (excess, unbounded)
    assert np.abs(h_gpu - h_ref).sum() <= max(4, 0.005 * h_ref.sum()), (np.abs(h_gpu - h_ref).sum(), h_ref.sum())


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("c", INIT, ids=lambda c: c.name)
def test_initialise_case_matches_oracle(c, state):
    st, tol = STATES[state]
    eng = engine(c, state=st)
    out, h = gpu_initialise(eng, c)
    ref, _, parts = oracle_initialise(c, h)
    assert_same_outcome(out, ref)
    print(f"{c.name} {state}: flag {out['flag_fail']}, {out['n_estimates']} poses, {out['n_candidates']} candidates")
    if out["found"]:
        dp = np.abs(np.asarray(out["predicted_pose"]) - np.asarray(ref["predicted_pose"])).max()
        ds = np.abs(eng.get_particles(1) - parts).max()
        print(f"{c.name} {state}: predicted_pose differs by {dp:.3g}, the seeded set by {ds:.3g}")
        assert dp <= 1e-9
        assert ds <= tol
    eng.close()


def test_particle_count_boundary():
    c = ic.boundary_case()
    eng = engine(c, N=64)
    out, h = gpu_initialise(eng, c, N=64)
    K = out["n_estimates"]
    assert out["found"] == 1 and K == oracle_initialise(c, h, N=64)[0]["n_estimates"]
    eng.close()
    for N, found in ((5, 0), (K + 1, 0), (K + 2, 1)):
        eng = engine(c, N=N)
        out, h = gpu_initialise(eng, c, N=N)
        ref, _, parts = oracle_initialise(c, h, N=N)
        assert_same_outcome(out, ref)
        assert out["found"] == found, (N, out)
        if found:
            np.testing.assert_allclose(eng.get_particles(1), parts, rtol=0, atol=1e-12)
        eng.close()


def test_candidate_cap_keeps_stage_one():
    c = ic.cap_case()
    eng = engine(c)
    with pytest.raises(pf.PFError) as e:
        pf.Engine.initialise_multi([eng], [c.blobs], n_particles=c.N, certainty_threshold=c.certainty_threshold,
                                   valid_corr_threshold=c.valid_corr_threshold, max_candidates=c.max_candidates)
    h = e.value.hist[0]
    assert np.array_equal(h, eng.p3p_histogram(c.blobs)) and h.sum() > 0
    with pytest.raises(RuntimeError):
        oracle_initialise(c, h)  # the oracle hits the same cap with that histogram
    with pytest.raises(pf.PFError):
        gpu_initialise(eng, c)
    eng.close()


@pytest.mark.parametrize("name", ["flag6", "flag7", "flag8", "flag11", "flag12"])
def test_not_found_leaves_the_prior_untouched(name):
    c = {k.name: k for k in INIT}[name]
    eng = engine(c, N=64)
    rng = np.random.default_rng(5)
    prior = np.tile(ic.syn.to12(ic.syn.truth_pose(0.2)), (64, 1)) + rng.normal(0, 1e-3, (64, 12))
    eng.set_prior(prior)
    before = eng.get_particles(1)
    out, _ = gpu_initialise(eng, c, N=64)
    assert out["found"] == 0
    assert np.array_equal(eng.get_particles(1), before)
    eng.close()


def test_mixed_batch_equals_its_singles():
    cases = [c for c in INIT if c.name in ("certainty_half_M6", "flag7", "valid_1.0", "collinear_model")]
    assert len(cases) == 4
    singles = []
    for c in cases:
        eng = engine(c)
        out, h = gpu_initialise(eng, c)
        singles.append((out, h, eng.get_particles(1) if out["found"] else None))
        eng.close()
    engs = [engine(c) for c in cases]
    res = pf.Engine.initialise_multi(engs, [c.blobs for c in cases], n_particles=[c.N for c in cases],
                                     certainty_threshold=[c.certainty_threshold for c in cases],
                                     valid_corr_threshold=[c.valid_corr_threshold for c in cases],
                                     max_candidates=[c.max_candidates for c in cases])
    for (out, h), (o1, h1, p1), eng in zip(res, singles, engs):
        assert_same_outcome(out, o1)
        assert np.array_equal(h, h1)
        assert np.array_equal(np.asarray(out["predicted_pose"]), np.asarray(o1["predicted_pose"]), equal_nan=True)
        if p1 is not None:
            assert np.array_equal(eng.get_particles(1), p1)
        eng.close()
