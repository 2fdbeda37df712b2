#!/usr/bin/env python3
"""Time the ROI prediction of S objects: (a) S sequential pfmpe_predict_roi calls against (b) one
pfmpe_predict_roi_multi, for S = 1, 4, 16 contexts of C2 size (100,000 fp32 particles) and S = 4 of C5 size (1M).

Both routes are blocking, so each is timed on the host around the calls, through ctypes with the argument arrays
built ahead: 5 warm-ups, then the median of 200 repetitions, the two routes alternating within one process.  Then the
batch alone, back to back ("alone": a loop of batches, whose members have no work on their own streams to be ordered
after), and a pass with PFMPE_OPT_TIMING on that reads the PFMPE_K_ROI device time of both routes (route (a): summed
over the S contexts).  Route (a) is S batches of one: the single call runs the batch's kernels and host path with one
stream (until it did, route (a) was a pair of kernels of its own and a copy back; DESIGN.md §4.14 has those figures).
Run it on an otherwise idle device.  Prints one row per case and one JSON line; exits non-zero unless the
batch is faster than the sequential calls for every S >= 4.

    python scripts/roi_multi_time.py [--cases C2:1,C2:4,C2:16,C5:4] [--warmup 5] [--reps 200]
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
from pf_monocular_pose_estimator_amd import _capi  # noqa: E402


def k_roi(eng):
    return list(eng.kernel_stats().values())[pf.K_ROI]


def run_case(name, S, warmup, reps):
    cfg = syn.CONFIGS[name]
    lib = pf.load()
    engs = []
    try:
        ins = []
        for s in range(S):
            st = syn.make_stream(syn.StreamConfig(name, M=cfg.M, B=cfg.B, N=cfg.N, seed=s), 1)
            eng = pf.Engine(device=0, max_particles=cfg.N, state_dtype=pf.STATE_F32)
            engs.append(eng)
            eng.set_model(st.markers, st.K)
            eng.set_prior(syn.initial_prior_fast(syn.to44(st.frames[0].current_pose), cfg.N, seed=7 + s))
            fr = st.frames[0]
            ins.append(pf.Engine.make_roi_in(fr.prediction, fr.predicted_pose, syn.D_README, syn.IMAGE_W, syn.IMAGE_H, 5))
        ctxs = (C.c_void_p * S)(*[e.ctx.value for e in engs])
        arr_in = (_capi.RoiIn * S)(*ins)
        out_a = (_capi.RoiOut * S)()
        out_b = (_capi.RoiOut * S)()
        refs_in = [C.byref(arr_in[s]) for s in range(S)]
        refs_out = [C.byref(out_a[s]) for s in range(S)]

        def route_a():
            for s in range(S):
                if lib.pfmpe_predict_roi(ctxs[s], refs_in[s], refs_out[s]) != pf.OK:
                    raise RuntimeError(engs[s].last_error())

        def route_b():
            if lib.pfmpe_predict_roi_multi(ctxs, S, arr_in, out_b) != pf.OK:
                raise RuntimeError(engs[0].last_error())

        for _ in range(warmup):
            route_a()
            route_b()
        ta, tb = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            route_a()
            t1 = time.perf_counter()
            route_b()
            t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e6)
            tb.append((t2 - t1) * 1e6)
        if bytes(out_a) != bytes(out_b):
            raise RuntimeError("the batch and the single calls disagree")
        # the batch alone, back to back (alternating, every batch first orders itself after the S - 1 single calls that
        # ran on the members' own streams: an event record and a stream wait each)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            route_b()
            ts.append((time.perf_counter() - t0) * 1e6)
        # device time of the PFMPE_K_ROI brackets, in a pass of its own (the brackets cost host time)
        dev_reps = max(reps // 4, 1)
        for e in engs:
            e.set_option(pf.OPT_TIMING, 1)
            e.reset_kernel_stats()
        for _ in range(dev_reps):
            route_a()
        dev_a = sum(k_roi(e)[1] for e in engs) / dev_reps * 1e3
        for e in engs:
            e.reset_kernel_stats()
        for _ in range(dev_reps):
            route_b()
        n_b, ms_b = k_roi(engs[0])
        dev_b = ms_b / max(n_b, 1) * 1e3
    finally:
        for e in engs:
            e.close()
    q = lambda v, p: float(np.percentile(v, p))  # noqa: E731
    return {"config": name, "S": S, "N": cfg.N, "reps": reps,
            "single_us": statistics.median(ta), "single_p10_us": q(ta, 10), "single_p90_us": q(ta, 90),
            "multi_us": statistics.median(tb), "multi_p10_us": q(tb, 10), "multi_p90_us": q(tb, 90),
            "multi_alone_us": statistics.median(ts), "single_device_us": dev_a, "multi_device_us": dev_b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2:1,C2:4,C2:16,C5:4")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    rows = []
    for case in args.cases.split(","):
        name, S = case.split(":")
        r = run_case(name, int(S), args.warmup, max(args.reps, 1))
        rows.append(r)
        print(f"{name} x {r['S']:2d}: N={r['N']}  {r['S']} x predict_roi {r['single_us']:8.1f} us "
              f"(p10 {r['single_p10_us']:.1f}, p90 {r['single_p90_us']:.1f}; device {r['single_device_us']:.1f})  "
              f"predict_roi_multi {r['multi_us']:8.1f} us (p10 {r['multi_p10_us']:.1f}, p90 {r['multi_p90_us']:.1f}; "
              f"device {r['multi_device_us']:.1f}; alone {r['multi_alone_us']:.1f})  "
              f"ratio {r['single_us'] / r['multi_us']:.2f}", flush=True)
    print(json.dumps({"roi_multi_time": rows}))
    return 0 if all(r["multi_us"] < r["single_us"] for r in rows if r["S"] >= 4) else 1


if __name__ == "__main__":
    sys.exit(main())
