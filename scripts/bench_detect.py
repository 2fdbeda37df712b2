"""Benchmark of the LED detector (led_detector.cpp:46-215): pfmpe_find_leds on a
device-resident 752x480 camera image (staged once: a camera DMA would land it there), full-image ROI and a
tracking-size ROI, against the CPU restatement (oracle/detect_oracle.cpp, 1 thread).  One JSON line.

  bench_detect.py [reps]            the single-ROI call, full image and tracking ROI
  bench_detect.py --multi R [reps]  R tracking-size ROIs: one pfmpe_find_leds_multi batch against R sequential
                                    pfmpe_find_leds calls on the same staged image"""
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


def main():
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
