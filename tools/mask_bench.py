"""Cost of a detection mask (detectAndComputeDevice with mask_ptr) against the
unmasked call on the same handle, both synchronous, on the C2 frame.

    python3 tools/mask_bench.py [--passes 5] [--calls 40] [--out profiles/mask/mask_bench.json]

One handle per (numFeatures, descriptor mode): 1920x1200, 3 octaves, the
bench.py frame in device memory; numFeatures 0 (OpenCV's keep-all: masked-out
keypoints are dropped before their orientation histogram) and 5000 (retainBest:
the mask acts in the order stage only).  Three legs per handle: no mask, an
all-255 mask and a mask that zeroes the right half of the frame.  Passes of
`calls` synchronous calls of each leg alternate (none, full, half, none, ...)
so that clock and neighbour drift hit all alike; each call is timed by the
host clock around the call and its sync.  Reported per handle: the median call
time of each pass, their median and range, and two ratios against the unmasked
leg of the same run:
    full_over_none   what carrying a mask costs (a masked frame launches the
                     detect chain eagerly, an unmasked one replays its graph)
    half_over_none   what masking half the frame saves; expected below 1 at
                     numFeatures 0, where half the orientation and descriptor
                     work disappears
Results are checked first: the masked legs must equal the unmasked result
filtered by sift_amd.cv.mask_keep.  Written as measured."""
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


def rows(det):
    det.copyToHost(True)
    return det.final_kpts.copy(), det.final_features.copy(), det.descriptors.view(np.uint16).copy()


def run(nfeat, exact, passes, calls):
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numFeatures=nfeat, numOctaves=3)
    det = sift.Detector(cfg, device=0, exact_descriptors=exact)
    det.gpuWarmUpAndAllocate()
    frame = sift.DeviceArray.from_numpy(sift.synth_frame(0, W, H))
    masks = {"full": np.full((H, W), 255, np.uint8), "half": np.full((H, W), 255, np.uint8)}
    masks["half"][:, W // 2:] = 0
    dmask = {k: sift.DeviceArray.from_numpy(m) for k, m in masks.items()}
    legs = {"none": lambda: det.detectAndComputeDevice(frame.value, W * 4),
            "full": lambda: det.detectAndComputeDevice(frame.value, W * 4, mask_ptr=dmask["full"].value, mask_stride=W),
            "half": lambda: det.detectAndComputeDevice(frame.value, W * 4, mask_ptr=dmask["half"].value, mask_stride=W)}
    legs["none"]()
    ref = rows(det)
    counts = {"none": len(ref[0])}
    for k in ("full", "half"):
        legs[k]()
        got = rows(det)
        keep = cv.mask_keep(ref[0][:, 0], ref[0][:, 1], masks[k])
        if any(a.tobytes() != b[keep].tobytes() for a, b in zip(got, ref)):
            raise SystemExit(f"the {k}-mask result differs from the filtered unmasked result: nothing to time")
        counts[k] = len(got[0])
    for _ in range(10):  # warm every leg
        for fn in legs.values():
            fn()
    ms = {k: [] for k in legs}
    for _ in range(passes):
        for k, fn in legs.items():
            ms[k].append(timed_calls(fn, calls))
    stages = {k: stage_split(det, fn, 10) for k, fn in legs.items()}
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"numFeatures": nfeat, "mode": "exact" if exact else "fast", "keypoints": counts}
    for k in legs:
        out[f"{k}_sync_ms"] = {"median": round(med(ms[k]), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4),
                               "passes": [round(x, 4) for x in ms[k]]}
    out["full_over_none"] = round(med(ms["full"]) / med(ms["none"]), 3)
    out["half_over_none"] = round(med(ms["half"]) / med(ms["none"]), 3)
    out["half_over_full"] = round(med(ms["half"]) / med(ms["full"]), 3)
    out["stage_ms_timing_mode"] = stages
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask", "mask_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("mask_bench needs a GPU: nothing is measured without one")
    res = {"workload": f"{W}x{H} f32 device frame, numOctaves=3, synth_frame(0); synchronous calls; masks: none, "
                       f"all-255, right half zero",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "runs": [run(nfeat, exact, a.passes, a.calls) for nfeat in (0, 5000) for exact in (False, True)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
