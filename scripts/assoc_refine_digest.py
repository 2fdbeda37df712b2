"""Digests of the association, refinement and top-K calls, one sha256 per raw output buffer, for comparing two builds
of the library bit for bit (run it on each build and diff the two outputs; profiles/assoc_single_as_batch/ holds such a
pair).

Calls: pfmpe_assoc_stats (the record and the votes table, with and without kDiagAssocDirect), pfmpe_get_pairs,
pfmpe_refine_cloud, pfmpe_refine_poses, pfmpe_refine_multi and pfmpe_top_particles with blobs, each on the POSTERIOR
and on the PROPAGATED set (refine_poses / refine_multi: on that set's first particles and their pairs) after one step.

Cases, all with the Philox generator.  Default: the three state types with pruning on and off at M = 5 / B = 50 /
N = 257 (a second block of one particle); fp32 state with pruning at N = 1 / B = 0, at N = 65,537 (a second chunk of
one row) / B = 1, and at N = 257 / B = 50 for M = 1, 8, 9, 13 (with 5: every marker bucket and both sides of its edges);
and the fp32 table of M = 16 / B = 1024, whose bins do not fit in LDS behind the blob table: 508 lines.  --full: every
state type and pruning option over N = 1, 257, 65,537 times B = 0, 1, 50 at M = 5 and over those four M, and the large
table: 3,280 lines, of which the default's are a subset.

    python scripts/assoc_refine_digest.py [--full]
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import _capi  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402

STATES = (("f64", pf.STATE_F64), ("f32", pf.STATE_F32), ("f16", pf.STATE_F16))
WHICH = (("posterior", pf.ASSOC_POSTERIOR), ("propagated", pf.ASSOC_PROPAGATED))
SHAPES = [(5, B, N) for N in (1, 257, 65_537) for B in (0, 1, 50)] + [(M, 50, 257) for M in (1, 8, 9, 13)]
BASE = (5, 50, 257)
F32_SHAPES = [(5, 0, 1), (5, 1, 65_537)] + [(M, 50, 257) for M in (1, 8, 9, 13)]  # default: fp32 with pruning only
HEAD = 64  # hypotheses of refine_poses / refine_multi
UP = C.POINTER(C.c_uint32)


def sha(*bufs):
    h = hashlib.sha256()
    for b in bufs:
        h.update(b if isinstance(b, bytes) else np.ascontiguousarray(b).tobytes())
    return h.hexdigest()


def assoc(eng, which, blobs):
    """The raw record and the raw votes table of one pfmpe_assoc_stats call."""
    ai, keep = eng._assoc_in(blobs, -1)
    out = _capi.AssocOut()
    votes = np.zeros(eng.M * (len(blobs) + 1), dtype=np.uint32)
    if eng.lib.pfmpe_assoc_stats(eng.ctx, which, C.byref(ai), C.byref(out), votes.ctypes.data_as(UP)) != pf.OK:
        raise RuntimeError(eng.last_error())
    return sha(bytes(out)), sha(votes)


def refined(d):
    out = {k: v for k, v in d.items() if k not in ("rows", "cov")}
    return sha(repr(sorted((k, np.asarray(v).tobytes()) for k, v in out.items())).encode()), sha(d["rows"]), sha(d["cov"])


def calls(eng, name, blobs):
    for wname, which in WHICH:
        at = f"{name} {wname}"
        for direct in (0, 1):
            eng.set_option(pf.OPT_DIAG, pf.DIAG_ASSOC_DIRECT if direct else 0)
            rec, votes = assoc(eng, which, blobs)
            print(f"{at} assoc_stats direct{direct} record {rec}")
            print(f"{at} assoc_stats direct{direct} votes {votes}")
        eng.set_option(pf.OPT_DIAG, 0)
        corr, n_corr = eng.get_pairs(which, blobs=blobs)
        print(f"{at} get_pairs corr {sha(corr)}")
        print(f"{at} get_pairs n_corr {sha(n_corr)}")
        for call, d in (("refine_cloud", eng.refine_cloud(which, blobs=blobs, want_cov=True)),
                        ("refine_poses", eng.refine_poses(eng.get_particles(which)[:HEAD], corr[:HEAD], blobs=blobs,
                                                          want_cov=True))):
            for part, digest in zip(("summary", "rows", "cov"), refined(d)):
                print(f"{at} {call} {part} {digest}")
        poses = eng.get_particles(which)
        half = min(len(poses), HEAD) // 2
        multi = pf.Engine.refine_multi([eng, eng], [poses[:half], poses[half:HEAD]], [corr[:half], corr[half:HEAD]],
                                       blobs_list=[blobs, blobs], want_cov=True)
        for s, d in enumerate(multi):
            for part, digest in zip(("summary", "rows", "cov"), refined(d)):
                print(f"{at} refine_multi entry{s} {part} {digest}")
    top = eng.top_particles(pf.TOP_BY_WEIGHT, K=8, blobs=blobs)
    for k in ("index", "key_value", "poses", "corr", "n_corr"):
        print(f"{name} top_particles {k} {sha(top[k])}")
    print(f"{name} top_particles record {sha(repr((top['n'], top['n_positive'], top['n_out'], top['n_examined'])).encode())}",
          flush=True)


def case(sname, state, prune, M, B, N):
    st = syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=N), 1)
    eng = pf.Engine(device=0, max_particles=N, state_dtype=state)
    try:
        eng.set_model(st.markers, st.K)
        prm = pf.default_params()
        prm.rng_mode = pf.RNG_PHILOX
        eng.set_params(prm)
        eng.set_option(pf.OPT_PRUNE, prune)
        eng.set_prior(syn.initial_prior_fast(syn.to44(st.frames[0].current_pose), N, seed=7))
        fr = st.frames[0]
        eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=900,
                                frame_idx=0))
        calls(eng, f"{sname}_prune{prune}_M{M}_B{B}_N{N}", fr.blobs)
    finally:
        eng.close()


def large_table():
    """M = 16, B = 1024 (tests/test_gpu_assoc.py test_direct_votes_large_table): every vote goes to the device table."""
    st = syn.make_stream(syn.StreamConfig("t", M=12, B=200, N=1000, heavy=True), 1)
    fr = st.frames[0]
    mk = syn.markers_16()
    rng = np.random.default_rng(3)
    true_px = syn.project(st.K, syn.to44(fr.current_pose), mk)
    near = true_px[rng.integers(0, 16, 400)] + rng.integers(1, 6, (400, 2)) * rng.choice([-1, 1], (400, 2))
    far = rng.uniform([0, 0], [syn.IMAGE_W, syn.IMAGE_H], size=(1024 - 16 - 400, 2))
    blobs = np.vstack([true_px, near, far])
    rng.shuffle(blobs)
    blobs = blobs.astype(np.float32).astype(np.float64)
    eng = pf.Engine(device=0, max_particles=1000, max_blobs=1024, state_dtype=pf.STATE_F32)
    try:
        eng.set_model(mk, st.K)
        eng.set_params(pf.default_params())
        eng.set_prior(st.prior(fast=True)[:1000])
        rec, votes = assoc(eng, pf.ASSOC_POSTERIOR, blobs)
        corr, n_corr = eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=blobs)
        print(f"f32_large_table assoc_stats record {rec}")
        print(f"f32_large_table assoc_stats votes {votes}")
        print(f"f32_large_table get_pairs corr {sha(corr)}")
        print(f"f32_large_table get_pairs n_corr {sha(n_corr)}", flush=True)
    finally:
        eng.close()


def main():
    full = "--full" in sys.argv[1:]
    for sname, state in STATES:
        for prune in (1, 0):
            for M, B, N in SHAPES:
                if full or (M, B, N) == BASE or (state == pf.STATE_F32 and prune == 1 and (M, B, N) in F32_SHAPES):
                    case(sname, state, prune, M, B, N)
    large_table()


if __name__ == "__main__":
    main()
