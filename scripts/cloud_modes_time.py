#!/usr/bin/env python3
"""Time pfmpe_cloud_modes(POSTERIOR) for K = 2 and K = 8 seeds against the routes it replaces, after one step at the
C2, C5 and C4 sizes: pfmpe_get_particles(1), the read-back a host-side clustering would start from, and K + 1 single
pfmpe_cloud_stats calls (what the reduction alone costs when it is not restricted to a mode).  The seeds are the K
best particles of the frame (pfmpe_top_particles, no suppression), so the modes interleave in memory: every wave of
every mode's entry has members, the costly case of the filtered reduction.

All calls are blocking, so each is timed on the host around the call: 5 warm-up calls, then the median of 20 (the
method of scripts/cloud_stats_time.py).  mode_of is not requested (nothing per particle crosses the host link); one
extra row times the call with it.  Run it on an otherwise idle device.  Prints one row per size and K, and one JSON
line.

    python scripts/cloud_modes_time.py [--sizes C2,C5,C4] [--ks 2,8] [--warmup 5] [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402
from cloud_stats_time import STATE, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="C2,C5,C4")
    ap.add_argument("--ks", default="2,8")
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
            eng.step(eng.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                    seed=1, frame_idx=0))
            buf = np.zeros((cfg.N, 12))
            bp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            t_read = median_ms(lambda: eng._chk(eng.lib.pfmpe_get_particles(eng.ctx, 1, bp)), args.warmup, args.reps)
            for K in [int(k) for k in args.ks.split(",")]:
                seeds = eng.top_particles(pf.TOP_BY_WEIGHT, K=K)["poses"]
                assert len(seeds) == K, "fewer than K particles with weight"

                def singles():
                    for s in list(seeds) + [seeds[0]]:
                        eng.cloud_stats(pf.CLOUD_POSTERIOR, s)

                t_modes = median_ms(lambda: eng.cloud_modes(pf.CLOUD_POSTERIOR, seeds, want_mode_of=False),
                                    args.warmup, args.reps)
                t_bytes = median_ms(lambda: eng.cloud_modes(pf.CLOUD_POSTERIOR, seeds), args.warmup, args.reps)
                t_single = median_ms(singles, args.warmup, args.reps)
                dicts, _ = eng.cloud_modes(pf.CLOUD_POSTERIOR, seeds, want_mode_of=False)
                rows.append({"config": name, "N": cfg.N, "K": K, "cloud_modes_ms": t_modes,
                             "cloud_modes_with_mode_of_ms": t_bytes, "get_particles_ms": t_read,
                             "single_stats_calls_ms": t_single, "members": [d["n"] for d in dicts]})
                print(f"{name}: N={cfg.N} K={K}  cloud_modes {t_modes:.4f} ms  with mode_of {t_bytes:.4f} ms  "
                      f"{K + 1} cloud_stats calls {t_single:.4f} ms  get_particles(1) {t_read:.3f} ms  "
                      f"members {[d['n'] for d in dicts]}", flush=True)
        finally:
            eng.close()
    print(json.dumps({"cloud_modes_time": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
