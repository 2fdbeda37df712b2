#!/usr/bin/env python3
"""Time the epilogue of a multi-object frame: the Gauss-Newton refinement of S objects' winners as ONE
pfmpe_refine_multi call, against the S blocking pfmpe_refine_poses calls it replaces.

Shape: 5 LEDs / 20 blobs (configuration A of tests/refine_ref.py: the synthetic scene at truth_pose(3.0)), K hypotheses
per stream with every LED paired, one context per stream.  Both columns are timed on the host around the C calls
themselves (the argument records are built once, outside the clock), rows and covariances requested: warm-up calls,
then the median.  Run it on an otherwise idle device.  Prints one row per shape and one JSON line.

    python scripts/refine_multi_time.py [--shapes 1x1,4x1,16x1,64x1,16x256] [--warmup 3] [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402

SCENE_T = 3.0
DP = C.POINTER(C.c_double)
U32 = C.POINTER(C.c_uint32)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def scene(n):
    """(markers, K, blobs, poses, pairs): n hypotheses around the truth pose with all 5 LEDs paired."""
    cfg = syn.StreamConfig("A", M=5, B=20, N=0)
    markers = syn.markers_for(5)
    T = syn.truth_pose(SCENE_T)
    blobs = syn.blobs_for_frame(cfg, T, 0, markers)
    cloud = syn.initial_prior(T, 8192, ang=0.002, trans=0.004)  # near the truth, as a frame's winner is
    eng = pf.Engine(device=0, max_particles=len(cloud), state_dtype=pf.STATE_F64)
    try:
        eng.set_model(markers, syn.K_README)
        eng.set_prior(cloud)
        poses = eng.get_particles(pf.ASSOC_POSTERIOR)
        pairs, n_corr = eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=blobs)
    finally:
        eng.close()
    sel = np.flatnonzero(n_corr == 5)
    if len(sel) == 0:
        raise SystemExit("no hypothesis with 5 pairs")
    sel = np.resize(sel, n)  # (repeated from the start when the cloud has fewer)
    return markers, syn.K_README.copy(), blobs, np.ascontiguousarray(poses[sel]), np.ascontiguousarray(pairs[sel])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1,4x1,16x1,64x1,16x256", help="S x K per stream, comma separated")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")]
    lib = pf.load()
    markers, Kc, blobs, poses, pairs = scene(max(S * K for S, K in shapes))
    out_rows = []
    for S, K in shapes:
        engs = []
        try:
            for _ in range(S):
                e = pf.Engine(device=0, max_particles=max(K, 16), state_dtype=pf.STATE_F32)
                e.set_model(markers, Kc)
                engs.append(e)
            ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engs])
            ins, outs = (pf.RefineIn * S)(), (pf.RefineOut * S)()
            ais, keep = [], []
            rows = [np.zeros(K, dtype=pf.REFINE_ROW_DTYPE) for _ in range(S)]
            covs = [np.zeros((K, 36)) for _ in range(S)]
            for s in range(S):
                ai, kb = pf.Engine._assoc_in(blobs, -1)
                po, pr = poses[s * K:(s + 1) * K], pairs[s * K:(s + 1) * K]
                keep.append((kb, po, pr))
                ais.append(ai)
                ins[s].blobs, ins[s].K = ai, K
                ins[s].poses, ins[s].corr = po.ctypes.data_as(DP), pr.ctypes.data_as(U32)
            rp = (C.c_void_p * S)(*[r.ctypes.data for r in rows])
            cp = (DP * S)(*[c.ctypes.data_as(DP) for c in covs])
            single_args = [(engs[s].ctx, C.byref(ais[s]), None, ins[s].poses, ins[s].corr, K, C.byref(outs[s]),
                            C.c_void_p(rows[s].ctypes.data), covs[s].ctypes.data_as(DP)) for s in range(S)]

            def batch():
                if lib.pfmpe_refine_multi(ctxs, S, ins, None, outs, rp, cp) != pf.OK:
                    raise RuntimeError(engs[0].last_error())

            def singles():
                for a in single_args:
                    if lib.pfmpe_refine_poses(*a) != pf.OK:
                        raise RuntimeError("pfmpe_refine_poses failed")

            t_single = median_ms(singles, args.warmup, args.reps)
            ref = b"".join(r.tobytes() + c.tobytes() for r, c in zip(rows, covs)) + bytes(outs)
            t_batch = median_ms(batch, args.warmup, args.reps)
            got = b"".join(r.tobytes() + c.tobytes() for r, c in zip(rows, covs)) + bytes(outs)
            iters = int(sum(o.iters_total for o in outs))
        finally:
            for e in engs:
                e.close()
        out_rows.append({"S": S, "K": K, "singles_ms": t_single, "batch_ms": t_batch, "ratio": t_single / t_batch,
                         "same_bytes": got == ref, "iters_mean": iters / (S * K)})
        print(f"S={S:3d} K={K:4d}: {S} x refine_poses {t_single:8.3f} ms, refine_multi {t_batch:8.3f} ms, "
              f"ratio {t_single / t_batch:6.2f}, same bytes {got == ref}, mean iterations {iters / (S * K):.1f}", flush=True)
    print(json.dumps({"refine_multi_time": out_rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
