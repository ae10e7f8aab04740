"""Cost of k nearest neighbours (Matcher.match_knn_*) against today's match_device (the price of K) and against the
only alternative a caller has without it, a torch fp32 GEMM of the rows plus torch.topk (what the feature buys),
2000 x 2000.

    python3 tools/match_knn_bench.py [--passes 5] [--calls 200] [--parent-lib PATH] [--out profiles/knn/match_knn_bench.json]

Two routes: detector buffers (two 1920x1200 frames, numFeatures 2000: the sidecar codes, no prep launch) and foreign
fp16 buffers holding the same rows (k_match_prep + k_match_knn; match_device converts inside k_match_single).  Legs per
route, each `calls` back-to-back calls on one stream between two HIP events, per call:
    match_device                today's top-2 (idx2, d2 written)
    knn_k2 / knn_k4 / knn_k8    match_knn_device
    knn_list_k4                 match_knn_list_device (k = 4, max_distance = the median 4th distance)
    knn_batched_p7_k8           match_knn_batched, 7 pairs of the same two sets, one call
    knn_7_singles_k8            7 match_knn_device calls
    gemm_topk8                  foreign route only: torch fp32 |q|^2 + |t|^2 - 2 q t^T and torch.topk(k = 8, smallest)
Passes of every leg alternate, so clock and neighbour drift hit all alike; reported per leg: the median of the pass
values and their range.  The bytes are checked before anything is timed: k-NN against sift_amd.cv.knn of the rows, its
first two columns against match_device, the list against sift_amd.cv.knn_records.

--parent-lib: a libsift_hip.so built from the parent commit.  match_device, match_guided_device and match_list_device
are then timed in child processes alternating between this build and that one (SIFT_HIP_LIB), one interleaved pair
per pass: their kernels are untouched, so the two should agree within the spread.  Written as measured."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
import sift_amd as sift  # noqa: E402

W, H, N = 1920, 1200, 2000
P = 7


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


def stream_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def summary(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
            "passes": [round(x, 2) for x in v]}


class Legs:
    def __init__(self, q, t, rows):
        import torch

        self.torch, self.q, self.t = torch, q, t
        self.m = sift.Matcher(N, N, max_pairs=P, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
        self.idx2, self.d2 = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32)
        self.idx, self.dk = torch.empty((P * N, 8), **i32), torch.empty((P * N, 8), **f32)
        self.recs, self.count = torch.empty((N * 8, 4), **i32), torch.empty(1, **i32)
        self.qf, self.tf = (r.view(torch.float16).float() for r in rows)
        self.cap = 0.0

    def match_device(self):
        self.m.match_device(self.q, N, self.t, N, 0.8, False, self.idx2.data_ptr(), self.d2.data_ptr(), 0, self.st)

    def knn(self, k):
        self.m.match_knn_device(self.q, N, self.t, N, k, self.idx.data_ptr(), self.dk.data_ptr(), self.st)

    def knn_list(self):
        self.m.match_knn_list_device(self.q, N, self.t, N, 4, self.recs.data_ptr(), self.count.data_ptr(), self.cap, self.st)

    def batched(self):
        self.m.match_knn_batched([self.q] * P, [N] * P, [self.t] * P, [N] * P, 8, self.idx.data_ptr(), self.dk.data_ptr(),
                                 self.st)

    def singles(self):
        for _ in range(P):
            self.knn(8)

    def gemm_topk(self):
        torch = self.torch
        D = (self.qf * self.qf).sum(1)[:, None] + (self.tf * self.tf).sum(1)[None, :] - 2.0 * (self.qf @ self.tf.T)
        return torch.topk(D, 8, dim=1, largest=False)

    def table(self, k):
        self.torch.cuda.synchronize()
        n = N * k
        return (self.idx.cpu().numpy().reshape(-1)[:n].reshape(N, k).copy(),
                self.dk.cpu().numpy().reshape(-1)[:n].reshape(N, k).copy())

    def check(self):
        """The bytes, before anything is timed."""
        from sift_amd import cv

        q, t = self.qf.cpu().numpy(), self.tf.cpu().numpy()
        ref = cv.knn(q, t, 8)
        self.match_device()
        self.torch.cuda.synchronize()
        top2 = (self.idx2.cpu().numpy(), self.d2.cpu().numpy())
        for k in (2, 4, 8):
            self.knn(k)
            gi, gd = self.table(k)
            if gi.tobytes() != np.ascontiguousarray(ref[0][:, :k]).tobytes() or \
                    gd.tobytes() != np.ascontiguousarray(ref[1][:, :k]).tobytes():
                raise SystemExit(f"k = {k}: the table differs from cv.knn: nothing to time")
            if k == 2 and (gi.tobytes() != top2[0].tobytes() or gd.tobytes() != top2[1].tobytes()):
                raise SystemExit("k = 2 differs from match_device: nothing to time")
        self.cap = float(np.median(np.sqrt(ref[1][:, 3])))
        self.knn_list()
        self.torch.cuda.synchronize()
        n = int(self.count.cpu()[0])
        exp = cv.knn_records(np.ascontiguousarray(ref[0][:, :4]), np.ascontiguousarray(ref[1][:, :4]), self.cap)
        got = self.recs.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n]
        if got.tobytes() != exp.tobytes() or not 0 < n < 4 * N:
            raise SystemExit("the k-NN list differs from cv.knn_records: nothing to time")
        self.batched()
        bi, bd = self.idx.cpu().numpy(), self.dk.cpu().numpy()
        for p in range(P):
            if bi[p * N:(p + 1) * N].tobytes() != ref[0].tobytes() or bd[p * N:(p + 1) * N].tobytes() != ref[1].tobytes():
                raise SystemExit(f"batched pair {p} differs from cv.knn: nothing to time")
        ti = self.gemm_topk()[1].cpu().numpy()
        return {"list_kept": n, "gemm_topk_rows_with_other_indices": int((ti != ref[0]).any(1).sum())}


def measure(legs, passes, calls, with_gemm):
    out = {"checks": legs.check()}
    names = [("match_device", legs.match_device), ("knn_k2", lambda: legs.knn(2)), ("knn_k4", lambda: legs.knn(4)),
             ("knn_k8", lambda: legs.knn(8)), ("knn_list_k4", legs.knn_list), ("knn_batched_p7_k8", legs.batched),
             ("knn_7_singles_k8", legs.singles)]
    if with_gemm:
        names.append(("gemm_topk8", legs.gemm_topk))
    for _ in range(20):
        for _k, fn in names:
            fn()
    legs.torch.cuda.synchronize()
    vals = {k: [] for k, _ in names}
    for _ in range(passes):
        for k, fn in names:
            vals[k].append(stream_us(legs.torch, fn, calls if "7" not in k else max(calls // 4, 10)))
    out["stream_us"] = {k: summary(v) for k, v in vals.items()}
    med = lambda k: out["stream_us"][k]["median"]  # noqa: E731
    out["knn_over_match_device"] = {k: round(med(k) / med("match_device"), 3) for k in ("knn_k2", "knn_k4", "knn_k8")}
    out["list_k4_minus_knn_k4_us"] = round(med("knn_list_k4") - med("knn_k4"), 2)
    out["batched_over_7_singles"] = round(med("knn_batched_p7_k8") / med("knn_7_singles_k8"), 3)
    if with_gemm:
        out["gemm_topk8_over_knn_k8"] = round(med("gemm_topk8") / med("knn_k8"), 3)
    return out


def child(calls):
    """The existing calls alone (this process's library: SIFT_HIP_LIB or the default build)."""
    import torch

    det, bufs, _keep = setup()
    q, t = bufs["detector"]
    fq, ft = bufs["foreign"]
    m = sift.Matcher(N, N, max_pairs=2, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    idx2, d2, match = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32), torch.empty(N, **i32)
    recs, count = torch.empty((N, 4), **i32), torch.empty(1, **i32)
    xy = det.device_kpts.data()  # positions of the current frame for both sides: the gate's cost, not its result
    legs = {
        "match_device_detector": lambda: m.match_device(q, N, t, N, 0.8, False, idx2.data_ptr(), d2.data_ptr(),
                                                        match.data_ptr(), st),
        "match_device_foreign": lambda: m.match_device(fq, N, ft, N, 0.8, False, idx2.data_ptr(), d2.data_ptr(),
                                                       match.data_ptr(), st),
        "match_guided_device": lambda: m.match_guided_device(q, N, t, N, xy, xy, 64.0, idx2_ptr=idx2.data_ptr(),
                                                             d2_ptr=d2.data_ptr(), match_ptr=match.data_ptr(), stream=st),
        "match_list_device": lambda: m.match_list_device(q, N, t, N, recs.data_ptr(), count.data_ptr(), st),
    }
    out = {"library": sift.version()}
    for name, fn in legs.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        out[name] = round(float(np.median([stream_us(torch, fn, calls) for _ in range(5)])), 2)
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
                raise SystemExit(f"child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
        print("pair", len(rows), json.dumps(pair), flush=True)
    out = {"pairs": rows}
    for leg in ("match_device_detector", "match_device_foreign", "match_guided_device", "match_list_device"):
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": summary(a), "parent_us": summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn", "match_knn_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("match_knn_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    _det, bufs, keep = setup()
    res = {"workload": f"{N} x {N} descriptors of two {W}x{H} synthetic frames (77, 78), numFeatures {N}; stream_us: "
                       f"{a.calls} back-to-back calls between HIP events, per call ({max(a.calls // 4, 10)} for the "
                       f"7-pair legs); {a.passes} interleaved passes, median of the pass values and their range",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "plan_splits": {"single": sift.Matcher.knn_plan(N, N, 1, 8), "p7": sift.Matcher.knn_plan(N, N, P, 8)},
           "routes": {}}
    for route in ("detector", "foreign"):
        q, t = bufs[route]
        res["routes"][route] = measure(Legs(q, t, keep), a.passes, a.calls, route == "foreign")
        print(route, json.dumps(res["routes"][route]), flush=True)
    if a.parent_lib:
        res["existing_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
