#!/usr/bin/env python3
"""Time pfmpe_assoc_stats after one step at the C2 and C3 sizes, with pfmpe_cloud_stats(POSTERIOR) on the same
context beside it as the yardstick (the other whole-set reduction of the resident prior), and pfmpe_get_pairs over the
whole set (the rows kernel with its read-back).

Every call is blocking, so each is timed on the host around the call: 5 warm-up calls, then the median of 20.  Run
it on an otherwise idle device.  Prints one row per size and one JSON line.

    python scripts/assoc_stats_time.py [--sizes C2,C3] [--warmup 5] [--reps 20] [--diag BITS]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="C2,C3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--diag", type=int, default=0, help="diagnostic switches set after the step (OPT_DIAG)")
    args = ap.parse_args()
    rows = []
    for name in args.sizes.split(","):
        cfg = syn.CONFIGS[name]
        st = syn.make_stream(cfg, 1)
        eng = pf.Engine(device=0, max_particles=cfg.N, state_dtype=pf.STATE_F32)
        try:
            eng.set_model(st.markers, st.K)
            prm = pf.default_params()
            prm.rng_mode = pf.RNG_PHILOX
            eng.set_params(prm)
            eng.set_prior(st.prior())
            fr = st.frames[0]
            out = eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                          seed=1, frame_idx=0))
            ref = np.array(out.winner_pose if out.resampled else out.most_likely_pose)
            eng.set_option(pf.OPT_DIAG, args.diag)
            t_post = median_ms(lambda: eng.assoc_stats(pf.ASSOC_POSTERIOR, blobs=fr.blobs), args.warmup, args.reps)
            t_prop = median_ms(lambda: eng.assoc_stats(pf.ASSOC_PROPAGATED, blobs=fr.blobs), args.warmup, args.reps)
            t_cloud = median_ms(lambda: eng.cloud_stats(pf.CLOUD_POSTERIOR, ref), args.warmup, args.reps)
            t_pairs = median_ms(lambda: eng.get_pairs(pf.ASSOC_POSTERIOR, blobs=fr.blobs), args.warmup, args.reps)
            t_pairs_prop = median_ms(lambda: eng.get_pairs(pf.ASSOC_PROPAGATED, blobs=fr.blobs), args.warmup, args.reps)
            a = eng.assoc_stats(pf.ASSOC_POSTERIOR, blobs=fr.blobs)
        finally:
            eng.close()
        rows.append({"config": name, "N": cfg.N, "M": cfg.M, "B": cfg.B, "diag": args.diag,
                     "resampled": int(out.resampled), "assoc_posterior_ms": t_post, "assoc_propagated_ms": t_prop,
                     "cloud_posterior_ms": t_cloud, "get_pairs_posterior_ms": t_pairs,
                     "get_pairs_propagated_ms": t_pairs_prop, "n_any": int(a["n_any"]),
                     "mode_share": [round(float(v) / cfg.N, 4) for v in a["mode_votes"]]})
        print(f"{name}: N={cfg.N} M={cfg.M} B={cfg.B}  assoc_stats(POSTERIOR) {t_post:.3f} ms  "
              f"assoc_stats(PROPAGATED) {t_prop:.3f} ms  cloud_stats(POSTERIOR) {t_cloud:.3f} ms  "
              f"get_pairs(POSTERIOR) {t_pairs:.3f} ms  get_pairs(PROPAGATED) {t_pairs_prop:.3f} ms", flush=True)
    print(json.dumps({"assoc_stats_time": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
