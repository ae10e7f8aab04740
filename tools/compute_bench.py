"""Descriptors for the frame's own keypoints (computeDevice) against the full
detect (detectAndComputeDevice), both synchronous, on the C2 frame.

    python3 tools/compute_bench.py [--passes 5] [--calls 40] [--out profiles/compute/compute_bench.json]

One handle per descriptor mode (1920x1200, 3 octaves, numFeatures 5000, the
bench.py frame).  The frame is detected once; its keypoints, copied to device
memory as 24-byte records, are what computeDevice describes.  Passes of
`calls` synchronous detect calls and `calls` synchronous compute calls
alternate (detect, compute, detect, ...) so that clock and neighbour drift hit
both alike; each call is timed by the host clock around the call and its
sync.  Reported per mode: the median call time of each pass, their median and
range, and the ratio compute / detect.  Then one timing-mode run of each chain
(set_timing: per-stage device events, eager launches) for the per-stage split.
The expectation: compute costs less than detect -- it drops extrema, refine,
orientation and order.  The compute chain launches eagerly where detect
replays a captured graph, so the dropped stages have to outweigh the launch
overhead of the pyramid's kernels; the result is written as measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
import sift_amd as sift  # noqa: E402
from sift_amd import cv  # noqa: E402

W, H = 1920, 1200


def timed_calls(fn, calls):
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return float(np.median(out)) * 1e3


def stage_split(det, fn, calls):
    det.set_timing(True)
    det.timing_reset()
    for _ in range(calls):
        fn()
    t = det.timing()
    det.set_timing(False)
    return {k: round(v["ms"] / calls, 4) for k, v in t.items() if v["launches"]}


def run(exact, passes, calls):
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numFeatures=5000, numOctaves=3)
    det = sift.Detector(cfg, device=0, exact_descriptors=exact)
    det.gpuWarmUpAndAllocate()
    frame = sift.DeviceArray.from_numpy(sift.synth_frame(0, W, H))
    det.detectAndComputeDevice(frame.value, W * 4)
    det.copyToHost(True)
    n = det.total_size
    want = det.descriptors.view(np.uint16).copy()
    kp = cv.keypoint_records(det.final_kpts, det.final_features)
    dk = sift.DeviceArray.from_numpy(kp)

    def detect():
        det.detectAndComputeDevice(frame.value, W * 4)

    def compute():
        det.computeDevice(frame.value, W * 4, dk.value, n)

    compute()
    det.copyToHost(True)
    if not np.array_equal(det.descriptors.view(np.uint16), want):
        raise SystemExit("compute's descriptors differ from detect's: nothing to time")
    for _ in range(10):  # warm both chains
        detect()
        compute()
    d_ms, c_ms = [], []
    for _ in range(passes):
        d_ms.append(timed_calls(detect, calls))
        c_ms.append(timed_calls(compute, calls))
    stages = {"detect": stage_split(det, detect, 10), "compute": stage_split(det, compute, 10)}
    med = lambda v: round(float(np.median(v)), 4)  # noqa: E731
    return {"mode": "exact" if exact else "fast", "keypoints": n,
            "detect_sync_ms": {"median": med(d_ms), "min": round(min(d_ms), 4), "max": round(max(d_ms), 4)},
            "compute_sync_ms": {"median": med(c_ms), "min": round(min(c_ms), 4), "max": round(max(c_ms), 4)},
            "compute_over_detect": round(float(np.median(c_ms)) / float(np.median(d_ms)), 3),
            "passes_detect_ms": [round(x, 4) for x in d_ms], "passes_compute_ms": [round(x, 4) for x in c_ms],
            "stage_ms_timing_mode": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compute", "compute_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("compute_bench needs a GPU: nothing is measured without one")
    res = {"workload": f"{W}x{H} f32 device frame, numOctaves=3, numFeatures=5000, synth_frame(0); synchronous calls",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "modes": [run(exact, a.passes, a.calls) for exact in (False, True)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
