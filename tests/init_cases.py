"""Builders of the (re)initialisation's envelope cases: inputs the brute-force P3P initialisation (pfmpe_init.hip) can
meet and tests/test_gpu_init.py never gives it.  tests/test_init_cases_host.py checks on the CPU, with the oracle, that
each case is what its name says; tests/test_gpu_init_envelope.py runs them on the device.

Every case is small enough for the oracle's histogram with its band to take under about 3 s of one CPU thread (the
band costs: 0.35 M solves/s against 0.9 M/s for the histogram alone), so C(B, 3) M (M - 1) (M - 2) stays below 1 M:
B = 15 at M = 13 and, stage 1 alone, B = 12 at M = 16.
"""
from dataclasses import dataclass, field

import numpy as np

from pf_monocular_pose_estimator_amd import synthetic as syn

# another camera than the README's: fx != fy, the principal point off the image centre
K_OTHER = np.array([[612.25, 0.0, 301.5], [0.0, 587.75, 255.125], [0.0, 0.0, 1.0]])

# five LEDs, the first three on one line: P3P's setup returns false for that triple, in both stages
MARKERS_COLLINEAR = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0], [0.05, 0.15, 0.02],
                              [0.12, -0.1, 0.06]])


@dataclass
class Case:
    name: str
    markers: np.ndarray
    blobs: np.ndarray
    K: np.ndarray = field(default_factory=lambda: syn.K_README.copy())
    tol: float = 5.0
    certainty_threshold: float = 1.0
    valid_corr_threshold: float = 0.5
    max_candidates: int = 1 << 20
    N: int = 200
    empty: bool = False  # the histogram is zero on both sides (no combination passes the spread filter)

    @property
    def M(self):
        return len(self.markers)

    @property
    def B(self):
        return len(self.blobs)


def f32(a):
    """Rounded through float32, as detector output is."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _std(name, M, n_out, seed, noise=0.0, near=0, **kw):
    blobs, _ = syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)
    return Case(name, syn.markers_for(M), blobs, **kw)


def histogram_cases():
    out = []
    # marker counts: one unused marker in the MAXU = 2 kernel; the first and the last of the widest bucket
    out.append(_std("M4", 4, 3, 0, 0.3))
    out.append(_std("M13", 13, 2, 1, 0.2))
    b, _ = syn.init_blobs(16, 0, 2, noise_px=0.2)
    out.append(Case("M16", syn.markers_for(16), b[:12]))  # 12 of the 16 detections: stage 1 alone runs with B < M
    # M = B = 4: ">= 5 blobs near the centroid" can never hold
    out.append(_std("M4_B4", 4, 0, 3, 0.0, empty=True))
    # the pruning window follows tol
    out.append(_std("tol1", 5, 3, 4, 0.4, near=1, tol=1.0))
    out.append(_std("tol12", 5, 3, 4, 0.4, near=1, tol=12.0))
    # another camera: blobs projected under it
    mk = syn.markers_for(6)
    T = syn.truth_pose(0.8)
    rng = np.random.default_rng(77)
    px = syn.project(K_OTHER, T, mk) + rng.normal(0.0, 0.2, (6, 2))
    px = np.vstack([px, [[120.5, 400.25], [560.0, 88.75]]])
    out.append(Case("other_camera", mk, f32(px), K=K_OTHER.copy()))
    # two blobs with equal x (the sorted list's tie), two identical blobs (the NaN path)
    b, _ = syn.init_blobs(5, 3, 5, noise_px=0.3)
    b = b.copy()
    b[6, 0] = b[1, 0]
    out.append(Case("equal_x", syn.markers_for(5), b))
    b, _ = syn.init_blobs(5, 2, 6, noise_px=0.3)
    out.append(Case("identical_blobs", syn.markers_for(5), np.vstack([b, b[2:3]])))
    # negative and out-of-image coordinates
    b, _ = syn.init_blobs(5, 0, 7, noise_px=0.3)
    out.append(Case("outside_image", syn.markers_for(5), np.vstack([b, f32([[-30.5, 100.25], [800.75, -12.5], [900.25, 600.0]])])))
    # a pair exactly 1000 px apart passes "> threshDist"; one ulp beyond it does not
    out.append(pair_case("pair_1000px", 0))
    out.append(pair_case("pair_beyond_1000px", 1))
    # the centroid's count: exactly 5 blobs in range (the 5 LEDs, two blobs far away), and 4 (M = 4, two far away)
    far = np.array([[3000.0, 240.0], [-2500.0, 100.0]])
    b, _ = syn.init_blobs(5, 0, 9, noise_px=0.2)
    out.append(Case("centroid_5", syn.markers_for(5), np.vstack([b, far])))
    b, _ = syn.init_blobs(4, 0, 9, noise_px=0.2)
    out.append(Case("centroid_4", syn.markers_for(4), np.vstack([b, far]), empty=True))
    # three collinear LEDs of five
    out.append(collinear_case())
    return out


# five LEDs on a wide bar, the first two a metre apart: at a depth of fx / 1000 m they project 1000 px apart
MARKERS_WIDE = np.array([[-0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.3, 0.05], [0.1, -0.25, 0.1], [-0.2, 0.15, -0.05]])


def pair_case(name, ulps):
    """The detections of MARKERS_WIDE seen from 0.475 m, LED 1's placed at LED 0's + (1000, 0) exactly (a shift below a
    float32 ulp of the pixel) and then `ulps` ulps of a double farther.  The combinations that hold both score, so
    the histogram depends on which way "> threshDist" goes for that pair (asserted in tests/test_init_cases_host.py)."""
    T = np.eye(4)
    T[:3, 3] = [0.02, -0.01, syn.K_README[0, 0] / 1000.0]
    b = np.vstack([f32(syn.project(syn.K_README, T, MARKERS_WIDE)), [[300.5, 100.25], [610.0, 402.5]]])
    b[1] = b[0] + [1000.0, 0.0]
    for _ in range(ulps):
        b[1, 0] = np.nextafter(b[1, 0], np.inf)
    return Case(name, MARKERS_WIDE.copy(), b)


def collinear_case():
    px = syn.project(syn.K_README, syn.truth_pose(0.5), MARKERS_COLLINEAR)
    return Case("collinear_model", MARKERS_COLLINEAR.copy(), f32(np.vstack([px, [[200.5, 100.25], [610.0, 402.5]]])))


def initialise_cases():
    """Cases of the whole initialisation.  The flag each reaches is asserted in tests/test_init_cases_host.py."""
    out = []
    # certainty_threshold 0.5: partial minCoeff extraction and the smallest-error choice
    out.append(_std("certainty_half_M6", 6, 3, 2, 0.3, certainty_threshold=0.5))
    out.append(_std("certainty_half_M7", 7, 2, 3, 0.3, certainty_threshold=0.5))
    # valid_correspondence_threshold: 9 of 10 subsets valid passes 0.9 and fails 1.0; 8 of 10 fails 0.9
    out.append(_std("valid_0.9", 5, 3, 1, 0.3, tol=2.0, valid_corr_threshold=0.9))
    out.append(_std("valid_1.0", 5, 3, 1, 0.3, tol=2.0, valid_corr_threshold=1.0))
    out.append(_std("valid_0.9_below", 5, 3, 0, 0.3, tol=2.0, valid_corr_threshold=0.9))
    # the failure flags
    out.append(_std("flag11", 5, 2, 6, 1.5, near=1, tol=1.0))
    out.append(_std("flag6", 5, 2, 1, 1.5, near=1, tol=1.0))
    out.append(_std("flag7", 4, 3, 0, 0.3, tol=1.0, valid_corr_threshold=1.0))
    out.append(_std("flag8", 4, 2, 5, 1.5, near=1, valid_corr_threshold=1.0))
    out.append(_std("flag12", 4, 0, 3, 0.0))
    out.append(collinear_case())
    return out


EXPECTED_FLAGS = {"certainty_half_M6": 0, "certainty_half_M7": 0, "valid_0.9": 0, "valid_1.0": 8, "valid_0.9_below": 8,
                  "flag11": 11,
                  "flag6": 6, "flag7": 7, "flag8": 8, "flag12": 12}


def cap_case():
    """More candidate vectors than max_candidates: the call fails with E_CAP after stage 1."""
    return _std("cap", 6, 4, 0, 0.5, near=2, tol=1.0, max_candidates=4096)


def boundary_case():
    """The particle-count boundary: with K stored poses, N <= K + 1 is "not found" and N = K + 2 is found."""
    return _std("n_boundary", 5, 3, 0, 0.3)
