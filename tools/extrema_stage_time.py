"""Extrema and refine stage times of the C2 workload (1920x1200, 3 octaves,
numFeatures 5000) in timing mode, single frames and a 16-frame batch, for A/B
of library builds (SIFT_HIP_LIB).  One JSON line; profiles/thresholds/ab.json
holds interleaved runs of it.

    SIFT_HIP_LIB=path/to/libsift_hip.so python tools/extrema_stage_time.py   (tools/ab_build.sh builds one of a revision)
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "another-cuda-sift_amd"))
import numpy as np
import sift_amd as sift

w, h = 1920, 1200
out = {"lib": os.environ.get("SIFT_HIP_LIB", "default")}
cfg = sift.CudaSiftConfig(col_width=w, row_width=h, numOctaves=3, numFeatures=5000)
img = sift.synth_frame(0, w, h)
det = sift.Detector(cfg, device=0)
det.gpuWarmUpAndAllocate()
for _ in range(5):
    det.detectAndCompute(img)
det.set_timing(True)
det.timing_reset()
for _ in range(40):
    det.detectAndCompute(img)
t = det.timing()
out["single_us"] = {k: round(1000 * v["ms"] / max(v["launches"], 1), 3) for k, v in t.items() if "extrema" in k or "refine" in k}
det.set_timing(False)
n = 16
frames = np.stack([sift.synth_frame(i, w, h) for i in range(n)])
dev = sift.DeviceArray.from_numpy(frames)
bd = sift.Detector(cfg, device=0, batch=n)
bd.gpuWarmUpAndAllocate()
for _ in range(3):
    bd.detectBatchDevice(dev.value, n, w * 4, h * w * 4, sync=True)
bd.set_timing(True)
bd.timing_reset()
for _ in range(20):
    bd.detectBatchDevice(dev.value, n, w * 4, h * w * 4, sync=True)
t = bd.timing()
out["batch16_us"] = {k: round(1000 * v["ms"] / max(v["launches"], 1), 3) for k, v in t.items() if "extrema" in k or "refine" in k}
out["names"] = sorted(t)
print(json.dumps(out))
