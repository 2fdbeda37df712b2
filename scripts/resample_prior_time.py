#!/usr/bin/env python3
"""Time pfmpe_resample_prior against the route it replaces on the same build: pfmpe_get_particles(1), the index
computation on the host (pfmpe_host_resample_source and a numpy gather) and pfmpe_set_prior; with a mode filter the
host route also needs every particle's mode, so it starts with pfmpe_cloud_modes and its mode_of read-back.  The source
context has stepped once at its size; the new prior goes to a second context of the new size (a fork), so every
repetition reads the same set.

Shapes: C5 -> C2 (1M -> 100k, fp32), C4 -> C5 (10M -> 1M, fp16) and 100k -> 1M (C2 grown, fp32); each once with every
particle a member (K = 0) and once keeping the larger of the two modes about the frame's two best particles
(pfmpe_top_particles, K = 2, at least a quarter of the weighted cloud's extent apart where the frame has two such
hypotheses, else without suppression).

All calls are blocking, so each is timed on the host around the call: 5 warm-up calls, then the median of 20 (the
method of scripts/cloud_stats_time.py).  Run it on an otherwise idle device.  The byte model of the device call is the
stored row in and out (24 / 48 / 96 B each way) plus 4 B per owner index of a deferred prior, per new particle; the
K = 0 rows print the fraction of the 8 TB/s HBM peak that is.  Prints one row per shape and filter, and one JSON line.

    python scripts/resample_prior_time.py [--shapes C5:C2,C4:C5,C2:C5] [--warmup 5] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402
from cloud_stats_time import BYTES, HBM_BYTES_PER_S, STATE, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C5:C2,C4:C5,C2:C5")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rows = []
    for shape in args.shapes.split(","):
        a, b = shape.split(":")
        cfg, state, n_new = syn.CONFIGS[a], STATE[a], syn.CONFIGS[b].N
        st = syn.make_stream(cfg, 1)
        src = pf.Engine(device=0, max_particles=cfg.N, state_dtype=state)
        dst = pf.Engine(device=0, max_particles=n_new, state_dtype=state)
        try:
            src.set_model(st.markers, st.K)
            prm = pf.default_params()
            prm.rng_mode = pf.RNG_PHILOX
            src.set_params(prm)
            src.set_prior(st.prior())
            fr = st.frames[0]
            src.step(src.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt,
                                    seed=1, frame_idx=0))
            owners = src.info(pf.INFO_LAST_RESAMPLE) == pf.RESAMPLE_OWNERS and src.info(pf.INFO_LAST_SHAPE) == 0
            mt = src.cloud_stats(pf.CLOUD_WEIGHTED)["max_trans"] / 4
            seeds = src.top_particles(pf.TOP_BY_WEIGHT, K=2, min_trans=mt)["poses"]
            if len(seeds) < 2:  # no second hypothesis that far away: the two best particles, modes interleaved
                seeds = src.top_particles(pf.TOP_BY_WEIGHT, K=2)["poses"]
            assert len(seeds) == 2, "fewer than two particles with weight"
            dicts, _ = src.cloud_modes(pf.CLOUD_POSTERIOR, seeds, want_mode_of=False)
            mode = 0 if dicts[0]["n"] >= dicts[1]["n"] else 1

            def host_route(filtered):
                mode_of = src.cloud_modes(pf.CLOUD_POSTERIOR, seeds)[1] if filtered else None
                p = src.get_particles(1)
                source, _ = pf.host_resample_source(mode_of, mode, n_new, N=cfg.N)
                dst.set_prior(p[source])

            for filtered in (False, True):
                kw = dict(seeds=seeds, mode=mode) if filtered else {}
                out = dst.resample_prior(n_new, src=src, **kw)
                t_dev = median_ms(lambda: dst.resample_prior(n_new, src=src, **kw), args.warmup, args.reps)
                t_host = median_ms(lambda: host_route(filtered), args.warmup, args.reps)
                model = n_new * (2 * BYTES[state] + (4 if owners else 0))
                row = {"shape": shape, "N": cfg.N, "n_new": n_new, "state_bytes": BYTES[state], "owners": bool(owners),
                       "filtered": filtered, "n_members": out["n_members"], "resample_prior_ms": t_dev,
                       "host_route_ms": t_host, "model_bytes": model}
                text = (f"{shape}: {cfg.N} -> {n_new} ({BYTES[state]} B rows{', owners' if owners else ''})  "
                        f"{'mode ' + str(mode) + ' of 2' if filtered else 'K = 0'}  members {out['n_members']}  "
                        f"resample_prior {t_dev:.4f} ms  host route {t_host:.3f} ms  ({t_host / t_dev:.0f}x)")
                if not filtered:
                    row["hbm_fraction"] = model / (t_dev * 1e-3) / HBM_BYTES_PER_S
                    text += f"  model {model / 1e6:.1f} MB = {100 * row['hbm_fraction']:.1f} % of HBM peak"
                rows.append(row)
                print(text, flush=True)
        finally:
            src.close()
            dst.close()
    print(json.dumps({"resample_prior_time": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
