#!/usr/bin/env python3
"""Time pfmpe_refine_cloud over the whole posterior after one step at the C2 shape (5 LEDs, 50 blobs, 100k particles,
fp32 state): the summary alone, then with all N rows and covariances read back; beside them the oracle's optimisePose
on a sample of the same particles and pairs on one CPU core, scaled to N.

Every call is blocking, so each is timed on the host around the call: warm-up calls, then the median.  Run it on an
otherwise idle device.  --t0 moves the frame along the synthetic trajectory (the iteration counts depend on the pose:
see tests/refine_ref.py).  Prints one row per frame time and one JSON line.

    python scripts/refine_time.py [--config C2] [--t0 0.5,2.98] [--warmup 3] [--reps 10] [--sample 2000]
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
from oracle import pforacle as orc  # noqa: E402


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
    ap.add_argument("--config", default="C2")
    ap.add_argument("--t0", default="0.5,2.98")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=2000)
    args = ap.parse_args()
    cfg = syn.CONFIGS[args.config]
    rows = []
    for t0 in [float(x) for x in args.t0.split(",")]:
        st = syn.make_stream(cfg, 1, t0=t0)
        eng = pf.Engine(device=0, max_particles=cfg.N, state_dtype=pf.STATE_F32)
        try:
            eng.set_model(st.markers, st.K)
            prm = pf.default_params()
            prm.rng_mode = pf.RNG_PHILOX
            eng.set_params(prm)
            eng.set_prior(st.prior())
            fr = st.frames[0]
            eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=1,
                                    frame_idx=0))
            t_sum = median_ms(lambda: eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=fr.blobs, count=0), args.warmup, args.reps)
            t_rows = median_ms(lambda: eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=fr.blobs, want_cov=True), args.warmup,
                               args.reps)
            t_pairs = median_ms(lambda: eng.assoc_stats(pf.ASSOC_POSTERIOR, blobs=fr.blobs, want_votes=False),
                                args.warmup, args.reps)
            s = eng.refine_cloud(pf.ASSOC_POSTERIOR, blobs=fr.blobs, count=0)
            idx = np.linspace(0, cfg.N - 1, args.sample).astype(np.int64)
            poses = eng.get_particles(1)[idx]
            pairs = eng.get_pairs(1, blobs=fr.blobs)[0][idx]
        finally:
            eng.close()
        c0 = time.perf_counter()
        its = [orc.optimise_pose(st.markers, st.K, fr.blobs, pairs[i], poses[i])[2] for i in range(len(idx))]
        t_orc = (time.perf_counter() - c0) / len(idx) * cfg.N * 1e3
        rows.append({"config": cfg.name, "t0": t0, "N": cfg.N, "M": cfg.M, "B": cfg.B, "refine_summary_ms": t_sum,
                     "refine_rows_cov_ms": t_rows, "assoc_stats_ms": t_pairs, "oracle_cpu_ms_scaled": t_orc,
                     "oracle_sample": len(idx), "oracle_sample_mean_iters": float(np.mean(its)),
                     "n_with_pairs": s["n_with_pairs"], "n_converged": s["n_converged"], "n_cap_kept": s["n_cap_kept"],
                     "n_cap_reverted": s["n_cap_reverted"], "iters_mean": s["iters_total"] / max(s["n"], 1),
                     "iters_max": s["iters_max"], "best": s["best"], "best_pairs": int(s["best_row"]["n_pairs"]),
                     "best_rms_after": float(s["best_row"]["rms_after"])})
        print(f"{cfg.name} t0={t0}: refine_cloud(POSTERIOR) summary {t_sum:.3f} ms, with rows + cov {t_rows:.3f} ms "
              f"(assoc_stats {t_pairs:.3f} ms); oracle on one core {t_orc:.0f} ms for N; iterations mean "
              f"{rows[-1]['iters_mean']:.1f} max {s['iters_max']}; converged {s['n_converged']} cap kept "
              f"{s['n_cap_kept']} reverted {s['n_cap_reverted']} of {s['n_with_pairs']} with pairs", flush=True)
    print(json.dumps({"refine_time": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
