"""Cost of two-view verification (Verifier.verify_device: a fixed-budget RANSAC for the fundamental matrix on the
device) at 2000 matches x K hypotheses, K in {256, 1024, 4096}, and of the chain it closes.

    python3 tools/verify_bench.py [--passes 5] [--calls 200] [--parent-lib PATH] [--out profiles/verify/verify_bench.json]
    python3 tools/verify_bench.py --trace K [--calls 200]     (under a kernel trace: only verify_device calls, for the
                                                               per-kernel split)

The list: 1200 true pairs of a synthetic two-camera scene (1920 x 1200, focal length 1400, the second camera rotated a
little and moved by (0.6, 0.1, 0.15); positions rounded to the quarter pixel) and 800 pairs of unrelated uniform
positions, shuffled, indexing shuffled position arrays.  Legs, per K:
    v   verify_device          gather + K hypotheses + K x n score + select, mask and inlier list written
    s   score_device           gather + score alone, on the K hypotheses v solved (uploaded as the caller's own)
Each leg is timed as `calls` back-to-back calls on one stream between two HIP events, per call; passes of every leg
alternate (v256, s256, v1024, ...), so clock and neighbour drift hit all alike; reported per leg: the median of the
passes and their range.  The result is checked first: the record, the mask and the list must equal
sift_amd.cv.ransac_fundamental byte for byte.  predicate evaluations per second = K x n / the score's share of s
(s minus the gather, the gather timed as s at K = 1).

The chain, on 2000 x 2000 descriptors of two synthetic frames with uniform positions (the geometry is meaningless, the
work is the same), wall-clock per iteration, each iteration ending synchronised:
    chain_device   match_list_device -> verify_device (count read from the list's device counter) on one stream with
                   no host synchronisation in between, one read-back of the 52-byte result record, then
                   match_list_epipolar_device under the returned F
    chain_host     the same with the list taken through the host between the stages: the list's count read back,
                   verify_host (synchronous; result, records and mask to host memory), then a fresh
                   match_list_epipolar_device

--parent-lib: a libsift_hip.so built from the parent commit.  match_device and match_epipolar_device are then timed in
child processes alternating between this build and that one (SIFT_HIP_LIB), one interleaved pair per pass: nothing on
their path changed (match.hip takes the predicate from a shared header), so the ranges should overlap."""
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

W, H, N, N_IN = 1920, 1200, 2000, 1200
KS = (256, 1024, 4096)
MAX_ERROR = 1.5
INF = float("inf")


def scene():
    """(matches, q_xy, t_xy, planted): N records over (N, 2) float32 position arrays."""
    rng = np.random.default_rng(11)
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    rvec, t = np.array([0.02, -0.03, 0.01]), np.array([0.6, 0.1, 0.15])
    th = np.linalg.norm(rvec)
    k = rvec / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < N_IN:
        uv = rng.uniform(0, (W, H), (4 * N_IN, 2))
        z = rng.uniform(3.0, 8.0, len(uv))
        X = (np.linalg.inv(K) @ np.c_[uv, np.ones(len(uv))].T) * z
        Y = K @ (R @ X + t[:, None])
        s = (Y[:2] / Y[2]).T
        ok = ((s >= 0) & (s < (W, H))).all(1)
        a, b = np.r_[a, uv[ok]], np.r_[b, s[ok]]
    q_xy = rng.uniform(0, (W, H), (N, 2))
    t_xy = rng.uniform(0, (W, H), (N, 2))
    qrow, trow = rng.permutation(N), rng.permutation(N)
    q_xy[qrow[:N_IN]], t_xy[trow[:N_IN]] = a[:N_IN], b[:N_IN]
    order = rng.permutation(N)
    m = np.zeros(N, sift.DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["distance"] = qrow[order], trow[order], 1.0
    grid = lambda p: (np.rint(p * 4) / 4).astype(np.float32)  # noqa: E731
    return m, grid(q_xy), grid(t_xy), order < N_IN


class Legs:
    def __init__(self):
        import torch

        self.torch = torch
        self.m, self.q_xy, self.t_xy, self.planted = scene()
        self.dm = torch.from_numpy(self.m.view(np.int32).reshape(N, 4).copy()).cuda()
        self.dq, self.dt = torch.from_numpy(self.q_xy).cuda(), torch.from_numpy(self.t_xy).cuda()
        self.v = sift.Verifier(N, max(KS), device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.res = torch.zeros(13, dtype=torch.int32, device="cuda")
        self.out = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(max(KS), dtype=torch.int32, device="cuda")
        self.Fs = {}

    def verify(self, K):
        self.v.verify_device(self.dm.data_ptr(), 0, N, self.dq.data_ptr(), N, self.dt.data_ptr(), N, self.res.data_ptr(),
                             self.out.data_ptr(), self.cnt.data_ptr(), self.mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def score(self, K):
        self.v.score_device(self.dm.data_ptr(), 0, N, self.dq.data_ptr(), N, self.dt.data_ptr(), N,
                            self.Fs[max(K, min(KS))].data_ptr(), K, MAX_ERROR, self.counts.data_ptr(), 2, 2, self.st)

    def check(self, K):
        """The device's result against the numpy rule; keeps the solved hypotheses for the score leg."""
        from sift_amd import cv

        self.verify(K)
        samples, F, valid, counts = self.v.hypotheses()
        ref = cv.ransac_fundamental(self.m, self.q_xy, self.t_xy, MAX_ERROR, K, 0)
        rec = self.res.cpu().numpy().view(sift.VERIFY_RESULT_DTYPE)[0]
        n = int(self.cnt.cpu()[0])
        if (rec["F"].tobytes() != ref["F"].tobytes() or rec["hypothesis"] != ref["hypothesis"] or n != ref["inliers"]
                or F.tobytes() != ref["Fs"].tobytes() or not np.array_equal(counts, ref["counts"])
                or not np.array_equal(self.mask.cpu().numpy(), ref["mask"])
                or self.out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes() != ref["list"].tobytes()):
            raise SystemExit(f"K = {K}: the device result differs from the reference: nothing to time")
        self.Fs[K] = self.torch.from_numpy(F.copy()).cuda()
        self.score(K)
        self.torch.cuda.synchronize()
        if not np.array_equal(self.counts.cpu().numpy()[:K], ref["counts"]):
            raise SystemExit(f"K = {K}: score_device differs from the reference: nothing to time")
        mask = ref["mask"] != 0
        return {"hypothesis": int(ref["hypothesis"]), "inliers": int(ref["inliers"]),
                "valid_hypotheses": int(ref["valid_hypotheses"]),
                "planted_recovered": int((mask & self.planted).sum()), "outliers_admitted": int((mask & ~self.planted).sum())}

    def stream_us(self, fn, calls):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        self.torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3


def summary(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
            "passes": [round(x, 2) for x in v]}


def measure(passes, calls):
    legs = Legs()
    out = {"results": {str(K): legs.check(K) for K in KS}}
    names = [("gather_s1", lambda: legs.score(1))]
    for K in KS:
        names += [(f"v{K}", lambda K=K: legs.verify(K)), (f"s{K}", lambda K=K: legs.score(K))]
    for _ in range(20):
        for _, fn in names:
            fn()
    legs.torch.cuda.synchronize()
    t = {k: [] for k, _ in names}
    for _ in range(passes):
        for k, fn in names:
            t[k].append(legs.stream_us(fn, calls))
    out["stream_us"] = {k: summary(v) for k, v in t.items()}
    med = lambda k: out["stream_us"][k]["median"]  # noqa: E731
    out["score_evaluations_per_s"] = {
        str(K): round(K * N / max(med(f"s{K}") - med("gather_s1"), 1e-3) * 1e6, -6) for K in KS}
    return out


def chain(passes, calls):
    """The three-call chain against the same chain through the host, wall-clock us per iteration."""
    import torch

    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=N), device=0)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(77, W, H))
    det.detectAndCompute(sift.synth_frame(78, W, H))
    if min(det.prev_size, det.total_size) < N:
        raise SystemExit(f"the frames gave {det.prev_size} / {det.total_size} keypoints: not the {N} x {N} workload")
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    rng = np.random.default_rng(7)
    dxy = [torch.from_numpy((rng.random((N, 2)) * (W, H)).astype(np.float32)).cuda() for _ in range(2)]
    qxy, txy = dxy[0].data_ptr(), dxy[1].data_ptr()
    m, v, K = sift.Matcher(N, N, max_pairs=1, device=0), sift.Verifier(N, 1024, device=0), 1024
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    lst, cnt, res = torch.zeros((N, 4), **i32), torch.zeros(1, **i32), torch.zeros(13, **i32)
    out, ocnt = torch.zeros((N, 4), **i32), torch.zeros(1, **i32)
    rec = np.zeros(1, sift.VERIFY_RESULT_DTYPE)
    # the identity as F where the list supports no hypothesis (the epipolar gate refuses an all-zero F)
    usable = lambda F: F if np.any(F) else np.eye(3, dtype=np.float32)  # noqa: E731

    def device():
        m.match_list_device(q, N, t, N, lst.data_ptr(), cnt.data_ptr(), st)
        v.verify_device(lst.data_ptr(), cnt.data_ptr(), N, qxy, N, txy, N, res.data_ptr(), 0, 0, 0, MAX_ERROR, K, 0, 2, 2,
                        st)
        sift._check(sift.lib().sift_hip_memcpy_d2h(rec.ctypes.data, res.data_ptr(), 52), "d2h")  # the one read-back
        m.match_list_epipolar_device(q, N, t, N, qxy, txy, usable(rec["F"][0]), MAX_ERROR, out.data_ptr(), ocnt.data_ptr(),
                                     INF, 2, 2, st)
        torch.cuda.synchronize()

    def host():
        m.match_list_device(q, N, t, N, lst.data_ptr(), cnt.data_ptr(), st)
        n = int(cnt.cpu()[0])
        F, _inl, _hyp = v.verify_host(lst.data_ptr(), 0, n, qxy, N, txy, N, MAX_ERROR, K, 0, 2, 2)
        m.match_list_epipolar_device(q, N, t, N, qxy, txy, usable(F), MAX_ERROR, out.data_ptr(), ocnt.data_ptr(), INF, 2, 2,
                                     st)
        torch.cuda.synchronize()

    device()
    a = (out.cpu().numpy().tobytes(), int(ocnt.cpu()[0]), int(cnt.cpu()[0]))
    host()
    if a != (out.cpu().numpy().tobytes(), int(ocnt.cpu()[0]), int(cnt.cpu()[0])):
        raise SystemExit("the two chains disagree: nothing to time")
    for _ in range(20):
        device()
        host()
    t_us = {"chain_device": [], "chain_host": []}
    for _ in range(passes):
        for k, fn in (("chain_device", device), ("chain_host", host)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t_us[k].append((time.perf_counter() - t0) / calls * 1e6)
    res_ = {"putative_matches": a[2], "guided_matches": a[1], "hypotheses": K,
            "wall_us_per_iteration": {k: summary(x) for k, x in t_us.items()}}
    res_["host_over_device"] = round(res_["wall_us_per_iteration"]["chain_host"]["median"]
                                     / res_["wall_us_per_iteration"]["chain_device"]["median"], 3)
    return res_


def child(calls):
    """match_device and match_epipolar_device alone on detector buffers (this process's library)."""
    import torch

    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=N), device=0)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(77, W, H))
    det.detectAndCompute(sift.synth_frame(78, W, H))
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    rng = np.random.default_rng(7)
    dxy = [torch.from_numpy((rng.random((N, 2)) * (W, H)).astype(np.float32)).cuda() for _ in range(2)]
    m = sift.Matcher(N, N, max_pairs=1, device=0)
    st = torch.cuda.current_stream().cuda_stream
    idx2 = torch.empty((N, 2), dtype=torch.int32, device="cuda")
    d2 = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    F = np.float32([0, 0, 0.001, 0, 0, -0.7, -0.001, 0.7, 0.1])

    def a():
        m.match_device(q, N, t, N, 0.8, False, idx2.data_ptr(), d2.data_ptr(), 0, st)

    def e():
        m.match_epipolar_device(q, N, t, N, dxy[0].data_ptr(), dxy[1].data_ptr(), F, 4.0, INF, 2, 2, 0.8, False,
                                idx2.data_ptr(), d2.data_ptr(), 0, st)

    def stream_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    for _ in range(20):
        a()
        e()
    torch.cuda.synchronize()
    out = {"library": sift.version()}
    for k, fn in (("match_device", a), ("match_epipolar_device", e)):
        out[k] = round(float(np.median([stream_us(fn) for _ in range(5)])), 2)
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
                raise SystemExit(f"untouched-legs child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
    out = {"pairs": rows}
    for leg in ("match_device", "match_epipolar_device"):
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": summary(a), "parent_us": summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def trace(K, calls):
    legs = Legs()
    legs.check(K)
    for _ in range(calls):
        legs.verify(K)
    legs.torch.cuda.synchronize()
    print(f"TRACE K={K} calls={calls + 1}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify", "verify_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    if a.trace:
        trace(a.trace, a.calls)
        return
    res = {"workload": f"{N} matches ({N_IN} true pairs of a synthetic two-camera scene + {N - N_IN} pairs of unrelated "
                       f"positions, {W} x {H}), max_error {MAX_ERROR}, seed 0; stream_us: {a.calls} back-to-back calls "
                       f"between HIP events, per call",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls}
    res.update(measure(a.passes, a.calls))
    res["chain"] = chain(a.passes, a.calls)
    if a.parent_lib:
        res["untouched_legs_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
