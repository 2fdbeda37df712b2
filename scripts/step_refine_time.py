#!/usr/bin/env python3
"""Time a tracking frame with its refinement epilogue: the fused call (pfmpe_step_refine / pfmpe_step_refine_multi)
against the two blocking calls it replaces (pfmpe_step + pfmpe_refine_poses; pfmpe_step_multi + pfmpe_refine_multi).

Twin engines (same model, prior, Philox stream) walk the same synthetic stream, one with the two-call sequence and one
with the fused call, frame by frame in the same run; every frame's outputs (frame record, summary, row, covariance)
are compared and must be equal bytes.  Times are taken on the host clock around the C calls alone (the argument
records are built before the clock starts): warm-up frames, then the median.  Rows:

    C2     N = 100,000, M = 5, B = 50, F32 (k_frame2)         pfmpe_step + pfmpe_refine_poses
    batch  S = 4, 16, 64 streams x N = 2,048, F32             pfmpe_step_multi + pfmpe_refine_multi

and, on the C2 row, the tail's device time from the PFMPE_K_AUX bracket of a few more frames with PFMPE_OPT_TIMING on
(on a one-launch frame that bracket is the tail alone).  Run it on an otherwise idle device.  Prints one line per
row and one JSON line.

    python scripts/step_refine_time.py [--streams 4,16,64] [--warmup 3] [--reps 20]
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

DP = C.POINTER(C.c_double)
U32 = C.POINTER(C.c_uint32)
TIMED_EXTRA = 10  # frames run with PFMPE_OPT_TIMING for the tail's bracket


def engine(st, N, prior):
    e = pf.Engine(device=0, max_particles=N, state_dtype=pf.STATE_F32)
    e.set_model(st.markers, st.K)
    prm = pf.default_params()
    prm.rng_mode = pf.RNG_PHILOX
    e.set_params(prm)
    e.set_prior(prior)
    return e


def frame_in(e, fr):
    return e.make_frame(fr.current_pose, fr.predicted_pose, fr.prediction, blobs=fr.blobs, dt=fr.dt, seed=5,
                        frame_idx=fr.index)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def row_single(lib, N, M, B, warmup, reps, t0):
    st = syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=N), warmup + reps + TIMED_EXTRA, t0=t0)
    prior = st.prior(N)
    a, b = engine(st, N, prior), engine(st, N, prior)
    try:
        t_two, t_fused, t_step, t_ref, iters, same = [], [], [], [], [], True
        for fr in st.frames[:warmup + reps]:
            fa, fb = frame_in(a, fr), frame_in(b, fr)
            oa, ob, ga, gb = pf.FrameOut(), pf.FrameOut(), pf.RefineOut(), pf.RefineOut()
            ra, rb, ca, cb = pf.RefineRow(), pf.RefineRow(), np.zeros(36), np.zeros(36)
            ai = pf.AssocIn(fa.blobs, fa.B, -1)
            step_args = (a.ctx, C.byref(fa), C.byref(oa))
            ref_args = (a.ctx, C.byref(ai), None, oa.winner_pose, oa.corr, 1, C.byref(ga), C.addressof(ra), ca.ctypes.data_as(DP))
            fused_args = (b.ctx, C.byref(fb), None, C.byref(ob), C.byref(gb), C.byref(rb), cb.ctypes.data_as(DP))

            def step():
                if lib.pfmpe_step(*step_args) != pf.OK:
                    raise RuntimeError(a.last_error())

            def refine():
                if lib.pfmpe_refine_poses(*ref_args) != pf.OK:
                    raise RuntimeError(a.last_error())

            def fused():
                if lib.pfmpe_step_refine(*fused_args) != pf.OK:
                    raise RuntimeError(b.last_error())

            t_step.append(clock(step))
            t_ref.append(clock(refine))
            t_two.append(t_step[-1] + t_ref[-1])
            t_fused.append(clock(fused))
            iters.append(ga.iters_total)
            if oa.flag_fail != pf.FLAG_ACCEPTED:
                raise SystemExit("the stream lost track: the two-call sequence was built for an accepted frame")
            same = same and (bytes(oa), bytes(ga), bytes(ra), ca.tobytes()) == (bytes(ob), bytes(gb), bytes(rb), cb.tobytes())
        shape, fallbacks = b.info(pf.INFO_LAST_SHAPE), b.info(pf.INFO_TAIL_FALLBACKS)
        b.set_option(pf.OPT_TIMING, 1)
        b.reset_kernel_stats()
        for fr in st.frames[warmup + reps:]:
            b.step_refine(frame_in(b, fr))
        n_aux, ms_aux = b.kernel_stats()["aux"]
        fallbacks_all = b.info(pf.INFO_TAIL_FALLBACKS)
    finally:
        a.close()
        b.close()
    return {"row": "C2" if N == 100_000 else f"N={N}", "N": N, "two_call_ms": statistics.median(t_two[warmup:]),
            "fused_ms": statistics.median(t_fused[warmup:]), "step_ms": statistics.median(t_step[warmup:]),
            "refine_ms": statistics.median(t_ref[warmup:]), "gn_iters_mean": statistics.mean(iters[warmup:]),
            "same_bytes": same, "shape": shape,
            "tail_fallbacks": max(fallbacks, fallbacks_all), "tail_device_us": 1e3 * ms_aux / max(n_aux, 1),
            "tail_brackets": n_aux}


def row_batch(lib, S, N, M, B, warmup, reps, t0):
    sts = [syn.make_stream(syn.StreamConfig("t", M=M, B=B, N=N, seed=s), warmup + reps, t0=t0) for s in range(S)]
    priors = [st.prior(N) for st in sts]
    ea = [engine(st, N, p) for st, p in zip(sts, priors)]
    eb = [engine(st, N, p) for st, p in zip(sts, priors)]
    try:
        ca_ = (C.c_void_p * S)(*[e.ctx.value for e in ea])
        cb_ = (C.c_void_p * S)(*[e.ctx.value for e in eb])
        t_two, t_fused, t_step, t_ref, iters, same = [], [], [], [], [], True
        for f in range(warmup + reps):
            fa = (pf.FrameIn * S)(*[frame_in(e, st.frames[f]) for e, st in zip(ea, sts)])
            fb = (pf.FrameIn * S)(*[frame_in(e, st.frames[f]) for e, st in zip(eb, sts)])
            keep = [st.frames[f].blobs for st in sts]  # (the FrameIn copies hold pointers into make_frame's arrays)
            bl = [np.ascontiguousarray(k, dtype=np.float64) for k in keep]
            for s in range(S):
                fa[s].blobs = fb[s].blobs = bl[s].ctypes.data_as(DP)
            oa, ob = (pf.FrameOut * S)(), (pf.FrameOut * S)()
            ga, gb = (pf.RefineOut * S)(), (pf.RefineOut * S)()
            ra, rb = (pf.RefineRow * S)(), (pf.RefineRow * S)()
            cova, covb = np.zeros((S, 36)), np.zeros((S, 36))
            ins = (pf.RefineIn * S)()
            for s in range(S):
                ins[s].blobs = pf.AssocIn(fa[s].blobs, fa[s].B, -1)
                ins[s].poses = C.cast(C.addressof(oa[s]) + pf.FrameOut.winner_pose.offset, DP)
                ins[s].corr = C.cast(C.addressof(oa[s]) + pf.FrameOut.corr.offset, U32)
                ins[s].K = 1
            rp = (C.c_void_p * S)(*[C.addressof(ra[s]) for s in range(S)])
            cp = (DP * S)(*[cova[s].ctypes.data_as(DP) for s in range(S)])

            def step():
                if lib.pfmpe_step_multi(ca_, S, fa, oa) != pf.OK:
                    raise RuntimeError(ea[0].last_error())

            def refine():
                if lib.pfmpe_refine_multi(ca_, S, ins, None, ga, rp, cp) != pf.OK:
                    raise RuntimeError(ea[0].last_error())

            def fused():
                if lib.pfmpe_step_refine_multi(cb_, S, fb, None, ob, gb, rb, covb.ctypes.data_as(DP)) != pf.OK:
                    raise RuntimeError(eb[0].last_error())

            t_step.append(clock(step))
            t_ref.append(clock(refine))
            t_two.append(t_step[-1] + t_ref[-1])
            t_fused.append(clock(fused))
            iters.append(max(g.iters_total for g in ga))
            if any(o.flag_fail != pf.FLAG_ACCEPTED for o in oa):
                raise SystemExit("a stream lost track: the two-call sequence was built for accepted frames")
            same = same and (bytes(oa), bytes(ga), bytes(ra), cova.tobytes()) == (bytes(ob), bytes(gb), bytes(rb), covb.tobytes())
        fallbacks = sum(e.info(pf.INFO_TAIL_FALLBACKS) for e in eb)
    finally:
        for e in ea + eb:
            e.close()
    return {"row": f"{S}x{N}", "S": S, "N": N, "two_call_ms": statistics.median(t_two[warmup:]),
            "fused_ms": statistics.median(t_fused[warmup:]), "step_ms": statistics.median(t_step[warmup:]),
            "refine_ms": statistics.median(t_ref[warmup:]), "gn_iters_mean": statistics.mean(iters[warmup:]),
            "same_bytes": same, "tail_fallbacks": fallbacks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="4,16,64", help="batch rows: streams per batch, comma separated")
    ap.add_argument("--t0", type=float, default=0.5, help="the synthetic stream's start time (synthetic.make_stream)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lib = pf.load()
    rows = [row_single(lib, 100_000, 5, 50, args.warmup, args.reps, args.t0)]
    rows += [row_batch(lib, int(S), 2048, 5, 50, args.warmup, args.reps, args.t0) for S in args.streams.split(",") if S]
    for r in rows:
        extra = (f", shape {r['shape']}, tail {r['tail_device_us']:.1f} us on the device ({r['tail_brackets']} brackets)"
                 if "shape" in r else "")
        print(f"{r['row']:>8}: two calls {r['two_call_ms']:7.3f} ms (step {r['step_ms']:.3f} + refinement {r['refine_ms']:.3f}), fused {r['fused_ms']:7.3f} ms, ratio "
              f"{r['two_call_ms'] / r['fused_ms']:5.2f}, same bytes {r['same_bytes']}, tail fallbacks {r['tail_fallbacks']}, "
              f"Gauss-Newton iterations {r['gn_iters_mean']:.0f}{extra}",
              flush=True)
    print(json.dumps({"step_refine_time": rows}))
    return 0 if all(r["same_bytes"] and r["tail_fallbacks"] == 0 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
