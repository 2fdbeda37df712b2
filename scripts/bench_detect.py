"""Benchmark of the LED detector (led_detector.cpp:46-215): pfmpe_find_leds on a
device-resident 752x480 camera image (staged once: a camera DMA would land it there), full-image ROI and a
tracking-size ROI, against the CPU restatement (oracle/detect_oracle.cpp, 1 thread).  One JSON line.

  bench_detect.py [reps]            the single-ROI call, full image and tracking ROI
  bench_detect.py --multi R [reps]  R tracking-size ROIs: one pfmpe_find_leds_multi batch against R sequential
                                    pfmpe_find_leds calls on the same staged image
  bench_detect.py --streams S[,S...] [reps]
                                    S cameras, each with its own host image and one tracking ROI: one
                                    pfmpe_find_leds_streams batch against S sequential pfmpe_find_leds calls"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pf_monocular_pose_estimator_amd as pf  # noqa: E402
from pf_monocular_pose_estimator_amd import synthetic as syn  # noqa: E402


def bench_multi(R, reps, rounds=5):
    """R tracking-size ROIs of one staged image as one pfmpe_find_leds_multi batch and as R sequential
    pfmpe_find_leds calls, in this process, alternating (rounds x reps of each; medians over the rounds).  Wall times
    with the timing option off, the PFMPE_K_DETECT brackets (device time) in a pass of their own."""
    T = syn.truth_pose(0.5)
    img, ideal = syn.led_image(T, syn.markers_for(5), seed=1)
    eng = pf.Engine(device=0, max_particles=1000)
    eng.set_model(syn.markers_for(5), syn.K_README)
    eng.stage_image(img)
    x0, y0 = int(ideal[:, 0].min()) - 30, int(ideal[:, 1].min()) - 30
    w, h = int(ideal[:, 0].max()) + 30 - x0, int(ideal[:, 1].max()) + 30 - y0
    # the object's box and R - 1 boxes of the same size shifted over it and its surroundings: the same work each
    rois = [(min(x0 + 7 * (r % 8), img.shape[1] - w), min(y0 + 9 * (r // 8), img.shape[0] - h), w, h) for r in range(R)]
    name = "k_det (detector pipeline)"

    def batch():
        return eng.find_leds_multi(None, rois=rois, D=syn.D_README)

    def sequential():
        return [eng.find_leds(None, D=syn.D_README, roi=r) for r in rois]

    for a, b in zip(batch(), sequential()):  # warm-up, and the two paths agree
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for _ in range(5):
        batch(), sequential()
    wall = {"batch": [], "sequential": []}
    for _ in range(rounds):
        for key, fn in (("batch", batch), ("sequential", sequential)):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            wall[key].append((time.perf_counter() - t0) / reps * 1e6)
    dev = {}
    eng.set_option(pf.OPT_TIMING, 1)
    for key, fn in (("batch", batch), ("sequential", sequential)):
        eng.reset_kernel_stats()
        for _ in range(reps):
            fn()
        n, ms = eng.kernel_stats()[name]
        dev[key] = {"brackets_per_frame": n / reps, "device_us": ms / reps * 1e3}
    eng.set_option(pf.OPT_TIMING, 0)
    res = {"metric": "LED detector, R tracking-size ROIs per frame: one batch vs R sequential calls", "unit": "us/frame",
           "R": R, "reps": reps, "rounds": rounds, "image": [int(img.shape[1]), int(img.shape[0])], "roi_size": [w, h],
           "detections": [int(len(d[0])) for d in batch()]}
    for key in ("batch", "sequential"):
        res[key] = {"wall_us": float(np.median(wall[key])), "wall_us_rounds": [round(v, 2) for v in wall[key]], **dev[key]}
    res["value"] = res["batch"]["wall_us"]
    res["speedup_wall"] = res["sequential"]["wall_us"] / res["batch"]["wall_us"]
    print(json.dumps(res))
    eng.close()


def bench_streams(S, reps, rounds=5):
    """S cameras, each with its own 752x480 host image and one tracking ROI, in this process, alternating:
      batch       one pfmpe_find_leds_streams (the ROI crops go up through the pull kernel)
      batch_copy  the same with the crops sent by one async copy command (the A/B switch)
      seq_host    S pfmpe_find_leds calls with the host image (each uploads its whole image)
      seq_staged  S pfmpe_find_leds calls on images staged beforehand (no upload)
    Every path is the bare C calls on arguments built beforehand.  Wall times with the timing option off (medians of
    rounds x reps), the PFMPE_K_DETECT brackets (device time) in a pass of their own, the host time of the pack, and
    the bytes that cross the host link per frame."""
    from pf_monocular_pose_estimator_amd import _capi
    lib = pf.load()
    markers = syn.markers_for(5)
    T = syn.truth_pose(0.5)
    ideal = syn.project(syn.K_README, T, markers)
    x0, y0 = int(ideal[:, 0].min()) - 30, int(ideal[:, 1].min()) - 30
    roi = (x0, y0, int(ideal[:, 0].max()) + 30 - x0, int(ideal[:, 1].max()) + 30 - y0)
    imgs = [syn.led_image(T, markers, seed=1 + s)[0] for s in range(S)]
    engs = []
    for s in range(S):
        e = pf.Engine(device=0, max_particles=1000)
        e.set_model(markers, syn.K_README)
        engs.append(e)
    h, w = imgs[0].shape
    ims, keep = _capi.make_detect_images([(e.ctx, img, None) for e, img in zip(engs, imgs)])
    ps = _capi.make_detect_params([roi] * S, [syn.D_README] * S, [None] * S)
    idx = (C.c_int32 * S)(*range(S))
    blobs = np.zeros((S, pf.MAX_BLOBS, 2))
    dist = np.zeros((S, pf.MAX_BLOBS, 2), dtype=np.float32)
    outs = (pf.DetectOut * S)()
    bp, fp = blobs.ctypes.data_as(C.POINTER(C.c_double)), dist.ctypes.data_as(C.POINTER(C.c_float))
    row_b = [blobs[s].ctypes.data_as(C.POINTER(C.c_double)) for s in range(S)]
    row_f = [dist[s].ctypes.data_as(C.POINTER(C.c_float)) for s in range(S)]
    null = C.POINTER(C.c_uint8)()

    def ok(rc):
        if rc != pf.OK:
            raise RuntimeError("detector call failed: %d %s" % (rc, engs[0].last_error()))

    def batch():
        ok(lib.pfmpe_find_leds_streams(ims, S, idx, ps, S, bp, fp, pf.MAX_BLOBS, outs))

    def batch_copy():
        engs[0].set_option(pf.OPT_DIAG, pf.DIAG_DET_COPY)
        batch()
        engs[0].set_option(pf.OPT_DIAG, 0)

    def seq_host():
        for s in range(S):
            ok(lib.pfmpe_find_leds(engs[s].ctx, ims[s].image, w, h, w, C.byref(ps[s]), row_b[s], row_f[s], pf.MAX_BLOBS,
                                   C.byref(outs[s])))

    def seq_staged():
        for s in range(S):
            ok(lib.pfmpe_find_leds(engs[s].ctx, null, w, h, w, C.byref(ps[s]), row_b[s], row_f[s], pf.MAX_BLOBS,
                                   C.byref(outs[s])))

    paths = (("batch", batch), ("batch_copy", batch_copy), ("seq_host", seq_host), ("seq_staged", seq_staged))
    seq_host()  # stages every camera's image, for seq_staged
    snap = {}
    for key, fn in paths:  # warm-up, and the paths agree
        blobs[:] = 0
        fn()
        snap[key] = (blobs.copy(), [o.n for o in outs])
        assert snap[key][1] == snap["batch"][1] and np.array_equal(snap[key][0], snap["batch"][0]), key
    for _ in range(5):
        for _, fn in paths:
            fn()
    wall = {key: [] for key, _ in paths}
    for _ in range(rounds):
        for key, fn in paths:
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            wall[key].append((time.perf_counter() - t0) / reps * 1e6)
    name = "k_det (detector pipeline)"
    dev = {}
    for e in engs:
        e.set_option(pf.OPT_TIMING, 1)
    for key, fn in paths:
        for e in engs:
            e.reset_kernel_stats()
        for _ in range(reps):
            fn()
        st = [e.kernel_stats()[name] for e in engs]
        dev[key] = {"brackets_per_frame": sum(n for n, _ in st) / reps, "device_us": sum(ms for _, ms in st) / reps * 1e3}
    for e in engs:
        e.set_option(pf.OPT_TIMING, 0)
    crops = (_capi.DetectCrop * S)()
    nbytes = C.c_int64()
    ok(lib.pfmpe_host_detect_plan(ims, S, idx, ps, S, crops, C.byref(nbytes)))
    buf = np.zeros(max(nbytes.value, 1), dtype=np.uint8)
    bufp = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    t0 = time.perf_counter()
    for _ in range(reps):
        ok(lib.pfmpe_host_detect_pack(ims, S, idx, ps, S, crops, bufp, nbytes.value))
    pack_us = (time.perf_counter() - t0) / reps * 1e6
    res = {"metric": "LED detector, S cameras with one tracking ROI each: one streams batch vs S sequential calls",
           "unit": "us/frame", "S": S, "reps": reps, "rounds": rounds, "image": [w, h], "roi_size": [roi[2], roi[3]],
           "detections": snap["batch"][1], "host_plan_and_pack_us": pack_us,
           "link_bytes_per_frame": {"batch": nbytes.value, "seq_host": S * w * h, "seq_staged": 0}}
    for key, _ in paths:
        res[key] = {"wall_us": float(np.median(wall[key])), "wall_us_rounds": [round(v, 2) for v in wall[key]], **dev[key]}
    res["value"] = res["batch"]["wall_us"]
    res["speedup_wall_vs_seq_host"] = res["seq_host"]["wall_us"] / res["batch"]["wall_us"]
    res["speedup_wall_vs_seq_staged"] = res["seq_staged"]["wall_us"] / res["batch"]["wall_us"]
    print(json.dumps(res), flush=True)
    for e in engs:
        e.close()


def main():
    if "--streams" in sys.argv:  # bench_detect.py --streams S[,S...] [reps]
        i = sys.argv.index("--streams")
        for S in sys.argv[i + 1].split(","):
            bench_streams(int(S), int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 300)
        return None
    if "--multi" in sys.argv:  # bench_detect.py --multi R [reps]
        i = sys.argv.index("--multi")
        return bench_multi(int(sys.argv[i + 1]), int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 200)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    T = syn.truth_pose(0.5)
    img, ideal = syn.led_image(T, syn.markers_for(5), seed=1)
    eng = pf.Engine(device=0, max_particles=1000)
    eng.set_model(syn.markers_for(5), syn.K_README)
    eng.stage_image(img)
    x0, y0 = int(ideal[:, 0].min()) - 30, int(ideal[:, 1].min()) - 30
    roi = (x0, y0, int(ideal[:, 0].max()) + 30 - x0, int(ideal[:, 1].max()) + 30 - y0)
    res = {"metric": "LED detector frames/s (threshold + blur + contours + moments + undistort)", "unit": "frames/s",
           "image": [int(img.shape[1]), int(img.shape[0])], "roi_tracking": list(roi)}
    for name, r in (("full", None), ("roi", roi)):
        for _ in range(5):
            eng.find_leds(None, D=syn.D_README, roi=r)
        eng.set_option(pf.OPT_TIMING, 1)
        eng.reset_kernel_stats()
        t0 = time.perf_counter()
        for _ in range(reps):
            und, _, info = eng.find_leds(None, D=syn.D_README, roi=r)
        wall = (time.perf_counter() - t0) / reps
        n, ms = eng.kernel_stats()["k_det (detector pipeline)"]
        eng.set_option(pf.OPT_TIMING, 0)
        res[name] = {"wall_us": wall * 1e6, "device_us": ms / max(n, 1) * 1e3, "detections": int(len(und)),
                     "components": info["n_components"]}
    from oracle import pforacle as orc
    for name, r in (("full", None), ("roi", roi)):
        t0 = time.perf_counter()
        k = 5
        for _ in range(k):
            orc.find_leds(img, syn.K_README, syn.D_README, roi=r)
        res[name]["cpu_us"] = (time.perf_counter() - t0) / k * 1e6
    res["value"] = 1e6 / res["full"]["wall_us"]
    res["cpu_baseline"] = {"value": 1e6 / res["full"]["cpu_us"], "unit": "frames/s", "cores": 1, "kind": "port",
                           "sample": "5 full 752x480 frames, oracle/detect_oracle.cpp"}
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
