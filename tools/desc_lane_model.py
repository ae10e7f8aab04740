#!/usr/bin/env python3
"""Lane-slot model of k_descriptor<128>'s enumerated sample loop (CPU only).

    python3 tools/desc_lane_model.py [--frames 0 1] [--old-item 174 --new-item 151] > model.json

The kernel issues one sample-loop step per work item (two consecutive samples
of a window row) for all 64 lanes of a wave, so what it pays for is lane slots,
not valid samples.  For the oracle's keypoints of synth_frame(f) at C2
(1920x1200, 3 octaves, numFeatures 5000) this restates, in float32,

  * desc_job_of (keypoints.hip): window radius, cos/sin / hist_width, centre;
  * the rows' intervals (sift_desc_rows.h): desc_clip_interval's conservative
    bounds with the image clipping, and the exact interval of the oracle's bin
    test (found here by evaluating the test on the whole window);
  * the work split: items of 2 samples per row, 128 threads, either every
    thread looping ceil(N / 128) times ("ceil", the code before the exact
    enumeration) or the first N % 128 threads taking one item more
    ("balanced": a wave loops as long as its longest thread),

and prints, per keypoint and in total: valid samples, enumerated samples, item
slots (2 x items) and lane slots (2 x 64 x the steps of each of the two waves)
for the old enumeration (conservative rows, ceil) and the new one (exact rows,
balanced).  With the VALU instructions of one item (--old-item / --new-item,
from the kernel's ISA) it also gives the predicted ratio of the sample loop's
issued VALU instructions.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "another-cuda-sift_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

f32 = np.float32
D, KDT, ITEM, MAX_ROWS = 4, 128, 2, 127
LB, UB = f32(-1.0) - f32(1e-4), f32(D) + f32(1e-4)


def job_of(k, W, H):
    """desc_job_of: (cos_t, sin_t, ptx, pty, rows, cols, radius) of an oracle keypoint record."""
    octave = int(k["octave"]) & 255
    octave = octave if octave < 128 else octave - 256
    scale = f32(1.0 / (1 << octave)) if octave >= 0 else f32(1 << -octave)
    cols, rows = (W >> octave, H >> octave) if octave >= 0 else (W << -octave, H << -octave)
    size = f32(k["size"]) * scale
    ptx, pty = int(np.rint(f32(k["x"]) * scale)), int(np.rint(f32(k["y"]) * scale))
    angle = f32(360.0) - f32(k["angle"])
    if abs(angle - f32(360.0)) < np.finfo(f32).eps:
        angle = f32(0.0)
    hist_width = f32(3.0) * (size * f32(0.5))
    radius = int(np.rint(hist_width * f32(1.4142135623730951) * f32(D + 1) * f32(0.5)))
    radius = min(radius, int(np.sqrt(float(cols) * cols + float(rows) * rows)))
    arg = angle * f32(np.pi / 180)
    return f32(np.cos(float(arg))) / hist_width, f32(np.sin(float(arg))) / hist_width, ptx, pty, rows, cols, radius


def clip(lo, hi, s, b, R):
    """desc_clip_interval over all rows at once (b: one value per row)."""
    if abs(s) < f32(1e-12):
        return lo, np.where((b <= LB) | (b >= UB), lo - 1, hi)
    inv = f32(1.0) / s
    x1, x2 = (LB - b) * inv, (UB - b) * inv
    x1, x2 = np.minimum(x1, x2), np.maximum(x1, x2)
    x1, x2 = np.maximum(x1, f32(-R - 2)), np.minimum(x2, f32(R + 2))
    return np.maximum(lo, np.floor(x1).astype(np.int64) - 1), np.minimum(hi, np.ceil(x2).astype(np.int64) + 1)


def rows_of(job):
    """Per window row: (conservative length, exact length) of the enumerated interval."""
    cos_t, sin_t, ptx, pty, rows, cols, R = job
    i = np.arange(-R, R + 1)
    fi = i.astype(f32)
    lo0, hi0 = max(-R, 1 - ptx), min(R, cols - 2 - ptx)
    lo = np.full(len(i), lo0, np.int64)
    hi = np.where((pty + i <= 0) | (pty + i >= rows - 1), lo0 - 1, hi0).astype(np.int64)
    in_image_row = hi >= lo
    lo, hi = clip(lo, hi, sin_t, fi * cos_t + f32(D / 2 - 0.5), R)
    lo, hi = clip(lo, hi, cos_t, -fi * sin_t + f32(D / 2 - 0.5), R)
    cons = np.maximum(hi - lo + 1, 0)
    # the oracle's test on the whole window (desc_sample's float operations)
    j = np.arange(-R, R + 1)
    fj = j.astype(f32)[None, :]
    c_rot = fj * cos_t - (fi * sin_t)[:, None]
    r_rot = fj * sin_t + (fi * cos_t)[:, None]
    rbin, cbin = r_rot + f32(D / 2) - f32(0.5), c_rot + f32(D / 2) - f32(0.5)
    ok = (rbin > -1) & (rbin < D) & (cbin > -1) & (cbin < D) & in_image_row[:, None] & ((j >= lo0) & (j <= hi0))[None, :]
    exact = ok.sum(axis=1)
    # the accepted samples of a row are one interval inside the conservative one
    first, last = ok.argmax(axis=1), ok.shape[1] - 1 - ok[:, ::-1].argmax(axis=1)
    assert ((last - first + 1 == exact) | (exact == 0)).all(), "a row's accepted samples are not contiguous"
    assert (((j[first] >= lo) & (j[last] <= hi)) | (exact == 0)).all(), "conservative interval misses a sample"
    return cons, exact


def slots(lens, balanced):
    """(item slots, lane slots, steps of the longest thread) of one keypoint's rows."""
    n = int(((lens + ITEM - 1) // ITEM).sum())
    if balanced:
        q, rem = divmod(n, KDT)
        steps = [q + (1 if rem > w * 64 else 0) for w in range(KDT // 64)]
    else:
        run = -(-n // KDT)  # thread t takes items [t * run, t * run + run): a wave's first thread is its longest
        steps = [min(run, max(n - w * 64 * run, 0)) for w in range(KDT // 64)]
    return ITEM * n, ITEM * 64 * sum(steps), max(steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[0, 1])
    ap.add_argument("--old-item", type=int, default=174, help="VALU instructions of one item before")
    ap.add_argument("--new-item", type=int, default=151, help="VALU instructions of one item now")
    a = ap.parse_args()
    import oracle_binding as oracle
    import sift_amd as sift

    W, H = 1920, 1200
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=5000)
    tot = {"keypoints": 0, "raster_keypoints": 0, "valid_samples": 0,
           "old": {"enumerated_samples": 0, "item_slots": 0, "lane_slots": 0, "steps": 0},
           "new": {"enumerated_samples": 0, "item_slots": 0, "lane_slots": 0, "steps": 0}}
    for f in a.frames:
        kps, _ = oracle.detect_and_compute(sift.synth_frame(f, W, H), oracle.from_config(cfg))
        for k in kps:
            job = job_of(k, W, H)
            if 2 * job[-1] + 1 > MAX_ROWS:  # the raster path: not enumerated
                tot["raster_keypoints"] += 1
                continue
            cons, exact = rows_of(job)
            tot["keypoints"] += 1
            tot["valid_samples"] += int(exact.sum())
            for name, lens, balanced in (("old", cons, False), ("new", exact, True)):
                items, lanes, steps = slots(lens, balanced)
                t = tot[name]
                t["enumerated_samples"] += int(lens.sum())
                t["item_slots"] += items
                t["lane_slots"] += lanes
                t["steps"] += steps
    n, v = max(tot["keypoints"], 1), max(tot["valid_samples"], 1)
    out = {"command": "python3 tools/desc_lane_model.py --frames " + " ".join(map(str, a.frames)), "frames": a.frames,
           "keypoints": tot["keypoints"], "raster_keypoints": tot["raster_keypoints"],
           "valid_samples": tot["valid_samples"], "valid_samples_per_keypoint": round(tot["valid_samples"] / n, 1)}
    for name in ("old", "new"):
        t = tot[name]
        out[name] = {"enumeration": "conservative rows, ceil(N/128) steps for every thread" if name == "old"
                     else "exact rows, balanced runs",
                     "per_keypoint": {k: round(t[k] / n, 2) for k in ("enumerated_samples", "item_slots", "lane_slots", "steps")},
                     "over_valid_samples": {k: round(t[k] / v, 4) for k in ("enumerated_samples", "item_slots", "lane_slots")}}
    lanes = tot["new"]["lane_slots"] / max(tot["old"]["lane_slots"], 1)
    out["predicted"] = {"lane_slots_new_over_old": round(lanes, 4), "item_valu_old": a.old_item, "item_valu_new": a.new_item,
                        "sample_loop_valu_new_over_old": round(lanes * a.new_item / a.old_item, 4)}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
