"""Cost of RootSIFT rows: the detector norm (Detector(root_sift=True), fused into the descriptor kernels) against the
plain norm, against what it replaces, and the stand-alone transform against its byte floor.  C2 frame (1920x1200 f32
in device memory, 3 octaves, numFeatures 5000), synchronous calls timed by the host clock around call + sync.

    python3 tools/rootsift_bench.py [--passes 5] [--calls 40] [--parent-lib ab/parent.so] [--out profiles/rootsift/rootsift_bench.json]

Legs (passes of `calls` calls alternate between the variants of a leg, so drift hits all alike; per variant the
median call time of each pass, and the median / min / max over passes):
  norm      detectAndComputeDevice, root against plain handle of THIS build, both descriptor modes; the descriptor
            kernel's own time from the handle's stage timing (events around the un-graphed kernel).
  replace   per frame pair: what a caller does to match RootSIFT rows of consecutive frames --
              fused   root handle: frame, then match prev x cur (both carry a sidecar: the direct path)
              device  plain handle: frame, rootsift_device in place on mutable_data(), match (converts: no sidecar)
              host    plain handle: frame, D2H, cv.rootsift, H2D into mutable_data(), match (converts)
            The three give the same match result (checked first).
  kernel    rootsift_device at 2,000 and 65,536 rows, out of place, `launches` launches between two syncs; against
            the byte floor n * 512 B at the measured HBM rate of bench.py's roofline leg (README Results).
  parent    with --parent-lib (tools/ab_build.sh HEAD~ parent): `pairs` interleaved process pairs, this build and the
            parent's, each running the plain norm leg (sync frame and descriptor stage time, both modes).
Not measured here: occupancy or any counter, more than one GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
import sift_amd as sift  # noqa: E402
from sift_amd import cv  # noqa: E402

W, H = 1920, 1200
HBM_MEASURED_GBS = (3790.0, 3920.0)  # bench.py roofline leg, box to box (README Results)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "passes": [round(x, 4) for x in v]}


def timed_calls(fn, calls):
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return float(np.median(out)) * 1e3


def interleaved(legs, passes, calls, warm=10):
    for _ in range(warm):
        for fn in legs.values():
            fn()
    ms = {k: [] for k in legs}
    for _ in range(passes):
        for k, fn in legs.items():
            ms[k].append(timed_calls(fn, calls))
    return ms


def desc_stage_ms(det, fn, calls=10):
    det.set_timing(True)
    det.timing_reset()
    for _ in range(calls):
        fn()
    t = det.timing()
    det.set_timing(False)
    return round(t["descriptor"]["ms"] / max(t["descriptor"]["launches"], 1), 4)


def detector(exact, root):
    cfg = sift.CudaSiftConfig(col_width=W, row_width=H, numFeatures=5000, numOctaves=3)
    kw = {"root_sift": True} if root else {}  # a parent build's package has no such argument
    det = sift.Detector(cfg, device=0, exact_descriptors=exact, **kw)
    det.gpuWarmUpAndAllocate()
    return det


def rows(det):
    det.copyToHost(True)
    return det.final_kpts.tobytes(), det.descriptors.astype(np.float32).astype(np.uint8)


def leg_norm(frame, passes, calls, with_root=True):
    out = []
    for exact in (False, True):
        dets = {"plain": detector(exact, False)}
        if with_root:
            dets["root"] = detector(exact, True)
        legs = {k: (lambda d=d: d.detectAndComputeDevice(frame.value, W * 4)) for k, d in dets.items()}
        for fn in legs.values():
            fn()
        res = {k: rows(d) for k, d in dets.items()}
        if with_root:
            if res["plain"][0] != res["root"][0] or not np.array_equal(cv.rootsift(res["plain"][1]), res["root"][1]):
                raise SystemExit("root rows differ from cv.rootsift(plain rows): nothing to time")
        ms = interleaved(legs, passes, calls)
        e = {"mode": "exact" if exact else "fast", "keypoints": len(res["plain"][1])}
        for k, d in dets.items():
            e[f"{k}_sync_ms"] = stats(ms[k])
            e[f"{k}_descriptor_kernel_ms"] = desc_stage_ms(d, legs[k])
        if with_root:
            e["root_over_plain"] = round(e["root_sync_ms"]["median"] / e["plain_sync_ms"]["median"], 4)
        out.append(e)
    return out


def leg_replace(frames, passes, calls):
    plain_d, plain_h, root = detector(False, False), detector(False, False), detector(False, True)
    cap = root.capacities()["results"]
    m = sift.Matcher(cap, cap)
    idx2, d2 = sift.DeviceArray(cap * 8), sift.DeviceArray(cap * 8)
    host = np.empty((cap, 128), np.uint16)
    turn = {"fused": 0, "device": 0, "host": 0}

    def match(det):
        m.match_device(det.prev_descriptor.data(), det.prev_size, det.device_descriptor.data(), det.total_size, 0.8, False,
                       idx2.value, d2.value)
        sift._check(sift.lib().sift_hip_device_sync(), "sync")

    def frame_of(k):
        turn[k] ^= 1
        return frames[turn[k]].value

    def fused():
        root.detectAndComputeDevice(frame_of("fused"), W * 4)
        match(root)

    def device():
        plain_d.detectAndComputeDevice(frame_of("device"), W * 4)
        sift.rootsift_device(plain_d.device_descriptor.mutable_data(), plain_d.total_size)
        match(plain_d)

    def via_host():
        det = plain_h
        det.detectAndComputeDevice(frame_of("host"), W * 4)
        n = det.total_size
        ptr = det.device_descriptor.mutable_data()
        sift._check(sift.lib().sift_hip_memcpy_d2h(host.ctypes.data, ptr, n * 256), "d2h")
        r = cv.rootsift(host[:n].view(np.float16)).astype(np.float16)
        sift._check(sift.lib().sift_hip_memcpy_h2d(ptr, r.ctypes.data, n * 256), "h2d")
        match(det)

    legs = {"fused": fused, "device": device, "host": via_host}
    got = {}
    for k, fn in legs.items():
        fn()
        fn()  # both frames transformed: prev x cur are root rows in every leg
        n = root.prev_size
        got[k] = idx2.to_numpy(np.int32, (cap, 2))[:n].copy(), d2.to_numpy(np.float32, (cap, 2))[:n].copy()
    for k in ("device", "host"):
        if not all(np.array_equal(a, b) for a, b in zip(got[k], got["fused"])):
            raise SystemExit(f"the {k} leg's match differs from the fused leg's: nothing to time")
    ms = interleaved(legs, passes, calls)
    out = {"rows": [root.prev_size, root.total_size], "per": "frame + transform + match of prev x cur, synchronous"}
    for k in legs:
        out[f"{k}_ms"] = stats(ms[k])
    out["fused_wholly_below_device"] = out["fused_ms"]["max"] < out["device_ms"]["min"]
    out["fused_wholly_below_host"] = out["fused_ms"]["max"] < out["host_ms"]["min"]
    return out


def leg_kernel(passes, launches):
    out = []
    rng = np.random.default_rng(3)
    for n in (2000, 65536):
        src = sift.DeviceArray.from_numpy(np.minimum(rng.exponential(30.0, (n, 128)), 255).astype(np.uint8).astype(np.float16))
        dst = sift.DeviceArray(n * 256)

        def burst():
            for _ in range(launches):
                sift.rootsift_device(src.value, n, dst.value)
            sift._check(sift.lib().sift_hip_device_sync(), "sync")

        burst()
        us = []
        for _ in range(passes):
            t = time.perf_counter()
            burst()
            us.append((time.perf_counter() - t) / launches * 1e6)
        floor = [n * 512 / (g * 1e3) for g in HBM_MEASURED_GBS[::-1]]  # us at the measured HBM rates
        out.append({"rows": n, "bytes": n * 512, "us_per_launch": stats(us),
                    "floor_us_at_measured_hbm": [round(f, 3) for f in floor],
                    "over_floor": round(float(np.median(us)) / floor[1], 1),
                    "note": "back-to-back launches between two syncs: launch-bound when far above the floor"})
    return out


def leg_parent(parent_lib, pairs, passes, calls):
    runs = {"this": [], "parent": []}
    for _ in range(pairs):
        for k, lib in (("this", None), ("parent", parent_lib)):
            env = dict(os.environ)
            env.pop("SIFT_HIP_LIB", None)
            if lib:
                env["SIFT_HIP_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--passes", str(passes), "--calls", str(calls)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{k} child failed: {r.stdout[-2000:]}{r.stderr[-2000:]}")
            runs[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"parent leg: {k} run {len(runs[k])} of {pairs}", file=sys.stderr, flush=True)
    out = {"pairs": pairs, "libraries": {k: v[0]["library"] for k, v in runs.items()}}
    for mode in (0, 1):
        e = {}
        for k, v in runs.items():
            sync = [x["norm"][mode]["plain_sync_ms"]["median"] for x in v]
            kern = [x["norm"][mode]["plain_descriptor_kernel_ms"] for x in v]
            e[k] = {"sync_ms": stats(sync), "descriptor_kernel_ms": stats(kern)}
        for q in ("sync_ms", "descriptor_kernel_ms"):
            e[f"{q}_ranges_overlap"] = e["this"][q]["min"] <= e["parent"][q]["max"] and e["parent"][q]["min"] <= e["this"][q]["max"]
        out["exact" if mode else "fast"] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true", help="the plain norm leg only, one JSON line (the parent leg's processes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rootsift", "rootsift_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("rootsift_bench needs a GPU: nothing is measured without one")
    frames = [sift.DeviceArray.from_numpy(sift.synth_frame(i, W, H)) for i in (0, 1)]
    if a.child:
        print(json.dumps({"library": sift.version(), "norm": leg_norm(frames[0], a.passes, a.calls, with_root=False)}))
        return
    res = {"workload": f"{W}x{H} f32 device frames, numOctaves=3, numFeatures=5000, synth_frame(0/1); synchronous calls",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "norm": leg_norm(frames[0], a.passes, a.calls),
           "replace": leg_replace(frames, a.passes, a.calls),
           "kernel": leg_kernel(a.passes, a.launches),
           "not_measured": "occupancy or any counter; more than one GPU"}
    if a.parent_lib:
        res["parent"] = leg_parent(a.parent_lib, a.pairs, 3, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
