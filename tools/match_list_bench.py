"""Cost of a match list (Matcher.match_list_device: match -> filter -> ordered compaction on the device) against
today's match_device and against the status quo a caller builds from it, 2000 x 2000.

    python3 tools/match_list_bench.py [--passes 5] [--calls 200] [--parent-lib PATH] [--out profiles/match_list/match_list_bench.json]

Two routes: detector buffers (two 1920x1200 frames, numFeatures 2000: the sidecar route, k_match_direct) and foreign
fp16 buffers holding the same rows (the converting kernels; with max_pairs = 1 two k_match_single launches, with
max_pairs = 2 one prep + one two-pair k_match_batch launch).  Legs per route:
    a  match_device                 today's top-2 + ratio test (idx2, d2 and match written)
    b  list, ratio only             match_list_device(cross_check=False): one direction + select
    c  list, cross_check            match_list_device(): both directions + select
    d  status quo                   two match_device calls, both top-2 arrays copied to the host,
                                    sift_amd.cv.filter_matches there (cross_check)
Each leg is timed two ways.  `stream_us`: `calls` back-to-back calls on one stream between two HIP events, per call
(the device cost; legs a-c).  `sync_us`: the host clock around ONE call and the synchronise that makes its result
usable (device sync for a-c -- the list stays on the device --, the finished host list for d), the median of `calls`
such calls.  Passes of every leg alternate (a, b, c, d, a, ...), so clock and neighbour drift hit all alike; reported
per leg: the median of the passes and their range.  Results are checked first: leg c's records must equal leg d's.

--parent-lib: a libsift_hip.so built from the parent commit.  match_device (leg a, both routes, and
`foreign_general`: the foreign rows halved, which takes the general fp16 path) is then timed in child processes
alternating between this build and that one (SIFT_HIP_LIB), one interleaved pair per pass: where its kernels are
untouched the two should agree within the spread.  Written as measured."""
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

W, H, N = 1920, 1200, 2000


def setup():
    import torch

    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=N), device=0)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(77, W, H))
    det.detectAndCompute(sift.synth_frame(78, W, H))
    n0, n1 = min(det.prev_size, N), min(det.total_size, N)
    if n0 < N or n1 < N:
        raise SystemExit(f"the frames gave {det.prev_size} / {det.total_size} keypoints: not the {N} x {N} workload")
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    foreign = []
    for src, n in ((q, n0), (t, n1)):
        rows = torch.empty((n, 128), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        sift._check(sift.lib().sift_hip_memcpy_d2d(rows.data_ptr(), src, n * 256, None), "d2d")
        foreign.append(rows)
    torch.cuda.synchronize()
    return det, {"detector": (q, t), "foreign": (foreign[0].data_ptr(), foreign[1].data_ptr())}, foreign


class Legs:
    """The four legs on one pair of buffers with one matcher configuration."""

    def __init__(self, q, t, max_pairs):
        import torch

        self.torch, self.q, self.t = torch, q, t
        self.m = sift.Matcher(N, N, max_pairs=max_pairs, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
        self.idx2, self.d2, self.match = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32), torch.empty(N, **i32)
        self.ridx2, self.rd2 = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32)
        self.recs, self.count = torch.empty((N, 4), **i32), torch.empty(1, **i32)
        self.host = [np.empty((N, 2), np.int32), np.empty((N, 2), np.float32), np.empty((N, 2), np.int32),
                     np.empty((N, 2), np.float32)]

    def a(self):
        self.m.match_device(self.q, N, self.t, N, 0.8, False, self.idx2.data_ptr(), self.d2.data_ptr(),
                            self.match.data_ptr(), self.st)

    def b(self):
        self.m.match_list_device(self.q, N, self.t, N, self.recs.data_ptr(), self.count.data_ptr(), self.st,
                                 cross_check=False)

    def c(self):
        self.m.match_list_device(self.q, N, self.t, N, self.recs.data_ptr(), self.count.data_ptr(), self.st)

    def d(self):
        from sift_amd import cv

        self.m.match_device(self.q, N, self.t, N, 0.8, False, self.idx2.data_ptr(), self.d2.data_ptr(), 0, self.st)
        self.m.match_device(self.t, N, self.q, N, 0.8, False, self.ridx2.data_ptr(), self.rd2.data_ptr(), 0, self.st)
        self.torch.cuda.synchronize()
        for dst, src in zip(self.host, (self.idx2, self.d2, self.ridx2, self.rd2)):
            sift._check(sift.lib().sift_hip_memcpy_d2h(dst.ctypes.data, src.data_ptr(), dst.nbytes), "d2h")
        return cv.filter_matches(*self.host)

    def list_c(self):
        self.c()
        self.torch.cuda.synchronize()
        n = int(self.count.cpu()[0])
        return self.recs.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n]

    def stream_us(self, fn, calls):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        self.torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    def sync_us(self, fn, calls, sync=True):
        out = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            if sync:
                self.torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return float(np.median(out)) * 1e6


def summary(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
            "passes": [round(x, 2) for x in v]}


def measure(legs, passes, calls):
    ref = legs.d()
    got = legs.list_c()
    if got.tobytes() != ref.tobytes():
        raise SystemExit("the cross-checked list differs from the status quo's: nothing to time")
    for _ in range(20):  # warm every leg
        for fn in (legs.a, legs.b, legs.c, legs.d):
            fn()
    legs.torch.cuda.synchronize()
    names = (("a_match_device", legs.a), ("b_list_ratio", legs.b), ("c_list_cross_check", legs.c), ("d_status_quo", legs.d))
    stream = {k: [] for k, _ in names[:3]}
    sync = {k: [] for k, _ in names}
    for _ in range(passes):
        for k, fn in names:
            if k in stream:
                stream[k].append(legs.stream_us(fn, calls))
            sync[k].append(legs.sync_us(fn, calls if k in stream else max(calls // 4, 10), sync=k in stream))
    out = {"kept": int(len(ref)), "stream_us": {k: summary(v) for k, v in stream.items()},
           "sync_us": {k: summary(v) for k, v in sync.items()}}
    med = lambda d, k: d[k]["median"]  # noqa: E731
    out["c_over_a_stream"] = round(med(out["stream_us"], "c_list_cross_check") / med(out["stream_us"], "a_match_device"), 3)
    out["c_minus_2a_stream_us"] = round(med(out["stream_us"], "c_list_cross_check") - 2 * med(out["stream_us"], "a_match_device"), 2)
    out["b_minus_a_stream_us"] = round(med(out["stream_us"], "b_list_ratio") - med(out["stream_us"], "a_match_device"), 2)
    out["d_over_c_sync"] = round(med(out["sync_us"], "d_status_quo") / med(out["sync_us"], "c_list_cross_check"), 3)
    return out


def child(calls):
    """match_device alone on both routes (this process's library: SIFT_HIP_LIB or the default build), and on the
    foreign rows halved (`foreign_general`: non-integer values, so the general fp16 path of k_match_single)."""
    import torch

    _det, bufs, _keep = setup()
    halved = [(rows.view(torch.float16) * 0.5).contiguous() for rows in _keep]
    torch.cuda.synchronize()
    bufs["foreign_general"] = (halved[0].data_ptr(), halved[1].data_ptr())
    out = {"library": sift.version()}
    for route, (q, t) in bufs.items():
        legs = Legs(q, t, 1)
        for _ in range(20):
            legs.a()
        legs.torch.cuda.synchronize()
        out[route] = round(float(np.median([legs.stream_us(legs.a, calls) for _ in range(5)])), 2)
    print("CHILD " + json.dumps(out), flush=True)


def parent_pairs(parent_lib, passes, calls):
    rows = []
    for _ in range(passes):
        pair = {}
        for name, libpath in (("this", None), ("parent", parent_lib)):
            env = dict(os.environ)
            env.pop("SIFT_HIP_LIB", None)
            if libpath:
                env["SIFT_HIP_LIB"] = libpath
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(calls)], env=env,
                               capture_output=True, text=True, timeout=600)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode or not line:
                raise SystemExit(f"match_device child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
    out = {"pairs": rows}
    for route in ("detector", "foreign", "foreign_general"):
        a, b = [p["this"][route] for p in rows], [p["parent"][route] for p in rows]
        out[route] = {"this_us": summary(a), "parent_us": summary(b),
                      "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_list", "match_list_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("match_list_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    _det, bufs, _keep = setup()
    res = {"workload": f"{N} x {N} descriptors of two {W}x{H} synthetic frames (77, 78), numFeatures {N}; stream_us: "
                       f"{a.calls} back-to-back calls between HIP events, per call; sync_us: host clock around one "
                       f"call and its synchronise (leg d: until the host list is ready)",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls, "routes": {}}
    for route, max_pairs in (("detector", 1), ("foreign", 1), ("foreign", 2)):
        q, t = bufs[route]
        name = route if route == "detector" else f"{route}_max_pairs_{max_pairs}"
        res["routes"][name] = measure(Legs(q, t, max_pairs), a.passes, a.calls)
    if a.parent_lib:
        res["match_device_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), min(a.passes, 3), a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
