#!/usr/bin/env python3
"""Time pfmpe_assoc_stats_multi(POSTERIOR) against S single pfmpe_assoc_stats calls in a loop: S objects of C2 size
(100k particles, 5 x 50) for S = 1, 8, 32 and 8 objects of C3 size (1M, 12 x 200), fp32 state, each after one step.

The method of scripts/assoc_stats_time.py: every call is blocking, so each is timed on the host around the call
(the loop: around all S calls), 5 warm-up calls, then the median of 20.  Run it on an otherwise idle device.  On a tree
without the batch call (the parent of the change that added it) the loop alone is timed.  Prints one row per case and
one JSON line.

    python scripts/assoc_multi_time.py [--cases C2x1,C2x8,C2x32,C3x8] [--warmup 5] [--reps 20]
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


def stepped(cfg, st, prior):
    eng = pf.Engine(device=0, max_particles=cfg.N, state_dtype=pf.STATE_F32)
    eng.set_model(st.markers, st.K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_PHILOX
    eng.set_params(prm)
    eng.set_prior(prior)
    fr = st.frames[0]
    eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=1,
                            frame_idx=0))
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2x1,C2x8,C2x32,C3x8")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    have_batch = hasattr(pf.Engine, "assoc_stats_multi")
    rows = []
    for case in args.cases.split(","):
        name, S = case.split("x")
        S = int(S)
        cfg = syn.CONFIGS[name]
        st = syn.make_stream(cfg, 1)
        prior = st.prior()
        blobs = st.frames[0].blobs
        engines = [stepped(cfg, st, prior) for _ in range(S)]
        try:
            def loop():
                return [e.assoc_stats(pf.ASSOC_POSTERIOR, blobs=blobs) for e in engines]

            def batch():
                return pf.Engine.assoc_stats_multi(engines, [pf.ASSOC_POSTERIOR] * S, [blobs] * S)

            t_loop = median_ms(loop, args.warmup, args.reps)
            t_batch = None
            if have_batch:
                t_batch = median_ms(batch, args.warmup, args.reps)
                for a, b in zip(loop(), batch()):
                    assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a), "batch != single calls"
        finally:
            for e in engines:
                e.close()
        rows.append({"case": case, "N": cfg.N, "M": cfg.M, "B": cfg.B, "S": S, "loop_ms": t_loop, "batch_ms": t_batch})
        tail = f"  one batch {t_batch:.3f} ms  ({t_loop / t_batch:.2f}x)" if have_batch else ""
        print(f"{case}: N={cfg.N} M={cfg.M} B={cfg.B}  {S} single calls {t_loop:.3f} ms{tail}", flush=True)
    print(json.dumps({"assoc_multi_time": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
