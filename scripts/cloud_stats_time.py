#!/usr/bin/env python3
"""Time pfmpe_cloud_stats(POSTERIOR) against the route it replaces, pfmpe_get_particles(1) (the N x 12 doubles a
host-side reduction would start from), after one step at the C2, C5 and C4 sizes; pfmpe_cloud_stats(WEIGHTED), which
regenerates the kept set first, is timed beside it.

Both calls are blocking, so each is timed on the host around the call: 5 warm-up calls, then the median of 20.  The
read-back writes into one preallocated buffer (no page faults of a fresh array in the timed calls).  Run it on an
otherwise idle device.  Prints one row per size and one JSON line.

    python scripts/cloud_stats_time.py [--sizes C2,C5,C4] [--warmup 5] [--reps 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402

STATE = {"C2": pf.STATE_F32, "C5": pf.STATE_F32, "C4": pf.STATE_F16}
BYTES = {pf.STATE_F32: 48, pf.STATE_F16: 24, pf.STATE_F64: 96}
HBM_BYTES_PER_S = 8e12


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
    ap.add_argument("--sizes", default="C2,C5,C4")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rows = []
    for name in args.sizes.split(","):
        cfg, state = syn.CONFIGS[name], STATE[name]
        st = syn.make_stream(cfg, 1)
        eng = pf.Engine(device=0, max_particles=cfg.N, state_dtype=state)
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
            buf = np.zeros((cfg.N, 12))
            bp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

            def read_back():
                eng._chk(eng.lib.pfmpe_get_particles(eng.ctx, 1, bp))

            t_stats = median_ms(lambda: eng.cloud_stats(pf.CLOUD_POSTERIOR, ref), args.warmup, args.reps)
            t_weighted = median_ms(lambda: eng.cloud_stats(pf.CLOUD_WEIGHTED, ref), args.warmup, args.reps)
            t_read = median_ms(read_back, args.warmup, args.reps)
            cs = eng.cloud_stats(pf.CLOUD_POSTERIOR, ref)
        finally:
            eng.close()
        floor_ms = cfg.N * BYTES[state] / HBM_BYTES_PER_S * 1e3
        rows.append({"config": name, "N": cfg.N, "state_bytes": BYTES[state], "resampled": int(out.resampled),
                     "cloud_stats_ms": t_stats, "cloud_stats_weighted_ms": t_weighted, "get_particles_ms": t_read,
                     "byte_floor_ms": floor_ms,
                     "ess": cs["ess"], "sigma_trans": float(np.sqrt(np.trace(cs["cov"][:3, :3]))),
                     "sigma_rot": float(np.sqrt(np.trace(cs["cov"][3:, 3:])))})
        print(f"{name}: N={cfg.N} {BYTES[state]} B/particle  cloud_stats {t_stats:.4f} ms  "
              f"weighted {t_weighted:.4f} ms  "
              f"get_particles(1) {t_read:.3f} ms  byte floor {floor_ms:.4f} ms", flush=True)
    print(json.dumps({"cloud_stats_time": rows}))
    return 0 if all(r["cloud_stats_ms"] < r["get_particles_ms"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
