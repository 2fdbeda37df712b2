"""Digests of the P3P (re)initialisation's outputs, one sha256 per case and output, for comparing two builds of the
library bit for bit (run it on each build and diff the two outputs; profiles/init_single_route/ holds such a pair).

Cases: the seven CASES of tests/test_gpu_init.py (pfmpe_p3p_histogram for all; pfmpe_initialise for the first four in the
three state types: the histogram, every pfmpe_init_out field and get_particles(1)), the slot-0 case with a prior
(K < N), the histogram-only calls below M (M = 5 at B = 3 and B = 4), and one histogram through the global-atomics path
(M = 12, B = 683: B x M x 4 bytes > 32 KB).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402

K = syn.K_README
N = 200
# tests/test_gpu_init.py's CASES: (M, uniform outliers, near outliers, seed, noise px)
CASES = [(5, 3, 0, 0, 0.0), (5, 10, 2, 1, 0.3), (8, 3, 0, 6, 0.0), (6, 4, 1, 9, 0.3), (5, 45, 0, 2, 0.3),
         (12, 3, 0, 3, 0.0), (12, 8, 4, 4, 0.3)]
STATES = (("f64", pf.STATE_F64), ("f32", pf.STATE_F32), ("f16", pf.STATE_F16))
OUT_KEYS = ("found", "flag_fail", "n_estimates", "n_candidates", "first_match", "hist_total")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def engine(M, max_particles, state=pf.STATE_F64):
    eng = pf.Engine(device=0, max_particles=max_particles, state_dtype=state)
    eng.set_model(syn.markers_for(M), K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_REFERENCE
    eng.set_params(prm)
    return eng


def out_digest(out):
    return sha(np.array([out[k] for k in OUT_KEYS], dtype=np.int64), np.asarray(out["pairs"], dtype=np.int64),
               np.asarray(out["predicted_pose"], dtype=np.float64))


def initialise_lines(name, eng, blobs, n):
    out, h = eng.initialise(blobs, n_particles=n)
    fields = " ".join(f"{k}={out[k]}" for k in OUT_KEYS)
    print(f"{name} hist {sha(h)}")
    print(f"{name} out {out_digest(out)} {fields}")
    print(f"{name} particles {sha(eng.get_particles(1))}")


def far_blobs(M, B):
    """The M projected markers and 3 outliers in the image, the rest on a line 1001 px apart: only the 3-blob
    combinations within the image pass the spread filter, so B can be large at a small cost."""
    near = syn.init_blobs(M, 3, seed=3)[0]
    far = np.array([[2000.0 + 1001.0 * k, 240.0] for k in range(B - len(near))])
    return np.vstack([near, far])


def main():
    for case in CASES:
        M, n_out, near, seed, noise = case
        blobs = syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)[0]
        name = f"M{M}_B{len(blobs)}_s{seed}"
        eng = engine(M, 256)
        print(f"{name} histogram {sha(eng.p3p_histogram(blobs))}")
        eng.close()
    for case in CASES[:4]:
        M, n_out, near, seed, noise = case
        blobs = syn.init_blobs(M, n_out, seed, noise_px=noise, near=near)[0]
        for sname, st in STATES:
            eng = engine(M, N, st)
            initialise_lines(f"M{M}_B{len(blobs)}_s{seed}_{sname}", eng, blobs, N)
            eng.close()
    # tests/test_gpu_init.py::test_initialise_keeps_resident_slot0
    eng = engine(5, 64)
    eng.set_prior(np.tile(syn.to12(syn.truth_pose(0.2)), (64, 1)))
    initialise_lines("slot0_prior_M5_N64", eng, syn.init_blobs(5, 2, 21)[0], 64)
    eng.close()
    b5 = syn.init_blobs(5, 0, 0)[0]
    for B in (3, 4):
        eng = engine(5, 64)
        h = eng.p3p_histogram(b5[:B])
        print(f"M5_B{B}_below_M histogram {sha(h)} total={int(h.sum())}")
        eng.close()
    eng = engine(12, 64)
    h = eng.p3p_histogram(far_blobs(12, 683))
    print(f"M12_B683_global_atomics histogram {sha(h)} total={int(h.sum())}")
    eng.close()


if __name__ == "__main__":
    main()
