"""Cost of the epipolar gate: the epipolar top-2 and cross-checked list (Matcher.match_epipolar_device,
Matcher.match_list_epipolar_device) against match_device and the window gate (match_guided_device) at the same shape
in the same run, 2000 x 2000, positions uniform in 1920 x 1200.

    python3 tools/match_epipolar_bench.py [--passes 5] [--calls 200] [--parent-lib PATH] [--out profiles/epipolar/match_epipolar_bench.json]

F is that of a synthetic pair (focal length 1400, principal point at the centre, the second camera rotated a little and
moved by (0.6, 0.1, 0.15)); max_error is found by bisection on sift_amd.cv.epipolar_mask so that a query has about as
many candidates in its band as in the window of radius 50 (2000 * (100 / 1920) * (100 / 1200) = 8.7).  Two routes, as
tools/match_guided_bench.py: detector buffers (the sidecar codes, one launch per direction) and foreign fp16 buffers
holding the same rows (k_match_prep first).  Legs per route:
    a   match_device                        top-2 + ratio test, no gate
    g   match_guided_device, radius 50      the window gate
    e   match_epipolar_device, band         about the window's candidate count
    ei  match_epipolar_device, max_error 1e30, radius inf: every row a candidate, the gate's arithmetic alone
    c   match_list_device                   cross-checked list, no gate
    h   match_list_guided_device, radius 50
    f   match_list_epipolar_device, band
Each leg is timed as `calls` back-to-back calls on one stream between two HIP events, per call.  Passes of every leg
alternate (a, g, e, ei, c, h, f, a, ...), so clock and neighbour drift hit all alike; reported per leg: the median of
the passes and their range.  Results are checked first: e and f must equal sift_amd.cv.epipolar_top2 / filter_matches
on the host copies (the reverse direction under F transposed), g sift_amd.cv.guided_top2, ei must equal a byte for byte.

--parent-lib: a libsift_hip.so built from the parent commit.  match_device and match_guided_device (both routes) are
then timed in child processes alternating between this build and that one (SIFT_HIP_LIB), one interleaved pair per
pass: both kernels are untouched, so the two builds should agree within the spread.  Written as measured."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
import sift_amd as sift  # noqa: E402

W, H, N, RADIUS = 1920, 1200, 2000, 50.0
INF = float("inf")


def fundamental():
    """F (float32, 3 x 3, unit Frobenius norm) of the synthetic pair: x_train^T F x_query = 0."""
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    rvec, t = np.array([0.02, -0.03, 0.01]), np.array([0.6, 0.1, 0.15])
    th = np.linalg.norm(rvec)
    k = rvec / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return (F / np.linalg.norm(F)).astype(np.float32)


def band_for(xy, F, target):
    """max_error (a float32 value) whose band holds about `target` train rows per query: bisection on the numpy rule."""
    from sift_amd import cv

    lo, hi = 0.01, 200.0
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        if cv.epipolar_mask(xy[0], xy[1], F, mid).sum(1).mean() < target:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


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
    rng = np.random.default_rng(7)
    xy = [(rng.random((N, 2)) * (W, H)).astype(np.float32) for _ in range(2)]
    dxy = [torch.from_numpy(a).cuda() for a in xy]
    host = [r.cpu().numpy().view(np.float16).astype(np.float32) for r in foreign]
    return det, {"detector": (q, t), "foreign": (foreign[0].data_ptr(), foreign[1].data_ptr())}, (foreign, dxy), xy, host


class Legs:
    def __init__(self, q, t, dxy, F=None, max_error=0.0):
        import torch

        self.torch, self.q, self.t, self.F, self.max_error = torch, q, t, F, max_error
        self.qxy, self.txy = dxy[0].data_ptr(), dxy[1].data_ptr()
        self.m = sift.Matcher(N, N, max_pairs=1, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
        self.idx2, self.d2, self.match = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32), torch.empty(N, **i32)
        self.recs, self.count = torch.empty((N, 4), **i32), torch.empty(1, **i32)

    def a(self):
        self.m.match_device(self.q, N, self.t, N, 0.8, False, self.idx2.data_ptr(), self.d2.data_ptr(),
                            self.match.data_ptr(), self.st)

    def guided(self, radius):
        self.m.match_guided_device(self.q, N, self.t, N, self.qxy, self.txy, radius, 2, 2, 0.8, False,
                                   self.idx2.data_ptr(), self.d2.data_ptr(), self.match.data_ptr(), self.st)

    def g(self):
        self.guided(RADIUS)

    def epipolar(self, max_error, radius=INF):
        self.m.match_epipolar_device(self.q, N, self.t, N, self.qxy, self.txy, self.F, max_error, radius, 2, 2, 0.8, False,
                                     self.idx2.data_ptr(), self.d2.data_ptr(), self.match.data_ptr(), self.st)

    def e(self):
        self.epipolar(self.max_error)

    def ei(self):
        self.epipolar(1e30)

    def f(self):
        self.m.match_list_epipolar_device(self.q, N, self.t, N, self.qxy, self.txy, self.F, self.max_error,
                                          self.recs.data_ptr(), self.count.data_ptr(), INF, 2, 2, self.st)

    def c(self):
        self.m.match_list_device(self.q, N, self.t, N, self.recs.data_ptr(), self.count.data_ptr(), self.st)

    def guided_list(self, radius):
        self.m.match_list_guided_device(self.q, N, self.t, N, self.qxy, self.txy, radius, self.recs.data_ptr(),
                                        self.count.data_ptr(), 2, 2, self.st)

    def h(self):
        self.guided_list(RADIUS)

    def top2(self, fn):
        fn()
        self.torch.cuda.synchronize()
        return self.idx2.cpu().numpy(), self.d2.cpu().numpy()

    def records(self, fn):
        fn()
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


def summary(v):
    return {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2),
            "passes": [round(x, 2) for x in v]}


def measure(legs, passes, calls, xy, host):
    from sift_amd import cv

    F, me = legs.F, legs.max_error
    fwd = cv.epipolar_top2(host[0], host[1], xy[0], xy[1], F, me)
    rev = cv.epipolar_top2(host[1], host[0], xy[1], xy[0], F.T, me)
    ref_list = cv.filter_matches(*fwd, *rev)
    got = legs.top2(legs.e)
    if got[0].tobytes() != fwd[0].tobytes() or got[1].tobytes() != fwd[1].tobytes():
        raise SystemExit("the epipolar top-2 differs from the reference: nothing to time")
    if legs.records(legs.f).tobytes() != ref_list.tobytes():
        raise SystemExit("the epipolar list differs from the reference: nothing to time")
    win = cv.guided_top2(host[0], host[1], xy[0], xy[1], RADIUS)
    got = legs.top2(legs.g)
    if got[0].tobytes() != win[0].tobytes() or got[1].tobytes() != win[1].tobytes():
        raise SystemExit("the guided top-2 differs from the reference: nothing to time")
    free, open_ = legs.top2(legs.a), legs.top2(legs.ei)
    if free[0].tobytes() != open_[0].tobytes() or free[1].tobytes() != open_[1].tobytes():
        raise SystemExit("every row a candidate differs from match_device: nothing to time")
    names = (("a_match_device", legs.a), ("g_guided_r50", legs.g), ("e_epipolar_band", legs.e),
             ("ei_epipolar_all", legs.ei), ("c_list_cross_check", legs.c), ("h_guided_list_r50", legs.h),
             ("f_epipolar_list_band", legs.f))
    for _ in range(20):  # warm every leg
        for _, fn in names:
            fn()
    legs.torch.cuda.synchronize()
    stream = {k: [] for k, _ in names}
    for _ in range(passes):
        for k, fn in names:
            stream[k].append(legs.stream_us(fn, calls))
    out = {"candidates_per_query_window": round(float(cv.gate_mask(xy[0], xy[1], RADIUS).sum(1).mean()), 2),
           "candidates_per_query_band": round(float(cv.epipolar_mask(xy[0], xy[1], F, me).sum(1).mean()), 2),
           "kept_epipolar_list": int(len(ref_list)), "stream_us": {k: summary(v) for k, v in stream.items()}}
    med = lambda k: out["stream_us"][k]["median"]  # noqa: E731
    out["e_over_a"] = round(med("e_epipolar_band") / med("a_match_device"), 3)
    out["e_over_g"] = round(med("e_epipolar_band") / med("g_guided_r50"), 3)
    out["ei_over_a"] = round(med("ei_epipolar_all") / med("a_match_device"), 3)
    out["f_over_c"] = round(med("f_epipolar_list_band") / med("c_list_cross_check"), 3)
    out["f_over_h"] = round(med("f_epipolar_list_band") / med("h_guided_list_r50"), 3)
    return out


def child(calls):
    """match_device and match_guided_device alone on both routes (this process's library: SIFT_HIP_LIB or the default
    build)."""
    _det, bufs, keep, _xy, _host = setup()
    out = {"library": sift.version()}
    for route, (q, t) in bufs.items():
        legs = Legs(q, t, keep[1])
        for _ in range(20):
            legs.a()
            legs.g()
        legs.torch.cuda.synchronize()
        out[route] = {k: round(float(np.median([legs.stream_us(fn, calls) for _ in range(5)])), 2)
                      for k, fn in (("match_device", legs.a), ("match_guided_device", legs.g))}
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
    for route in ("detector", "foreign"):
        out[route] = {}
        for leg in ("match_device", "match_guided_device"):
            a, b = [p["this"][route][leg] for p in rows], [p["parent"][route][leg] for p in rows]
            out[route][leg] = {"this_us": summary(a), "parent_us": summary(b),
                               "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                               "within_spread": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar", "match_epipolar_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("match_epipolar_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    _det, bufs, keep, xy, host = setup()
    from sift_amd import cv

    F = fundamental()
    max_error = band_for(xy, F, float(cv.gate_mask(xy[0], xy[1], RADIUS).sum(1).mean()))
    res = {"workload": f"{N} x {N} descriptors of two {W}x{H} synthetic frames (77, 78), numFeatures {N}; positions "
                       f"uniform in {W} x {H}; window radius {RADIUS:g}; F of a synthetic pair, max_error "
                       f"{max_error:.4g} (the window's candidate count) and 1e30; stream_us: {a.calls} back-to-back "
                       f"calls between HIP events, per call",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls, "F": [float(x) for x in F.reshape(-1)],
           "max_error": max_error, "routes": {}}
    for route in ("detector", "foreign"):
        q, t = bufs[route]
        res["routes"][route] = measure(Legs(q, t, keep[1], F, max_error), a.passes, a.calls, xy, host)
    if a.parent_lib:
        res["untouched_legs_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
