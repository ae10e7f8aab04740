"""Cost of k nearest neighbours inside a gate (Matcher.match_knn_guided_* / match_knn_epipolar_*) against the ungated
k-NN at the same k (the price or gain of the gate) and against the gated top-2 calls (the price of K under a gate),
2000 x 2000, positions uniform in 1920 x 1200.

    python3 tools/match_knn_gated_bench.py [--passes 5] [--calls 200] [--parent-lib PATH]
                                           [--out profiles/knn_gated/match_knn_gated_bench.json]

The window has radius 50, the band max_error 1.95 under the F of tools/match_epipolar_bench.py (about 8.5 candidates
per query each).  Two routes, as tools/match_knn_bench.py: detector buffers (the sidecar codes, no prep launch) and
foreign fp16 buffers holding the same rows (k_match_prep + k_match_knn).  Legs per route, each `calls` back-to-back
calls on one stream between two HIP events, per call:
    match_device, guided_top2, epipolar_top2         today's top-2 calls
    knn_k2 / k4 / k8                                 match_knn_device
    knn_guided_k2 / k4 / k8, knn_epipolar_k2 / k4 / k8
    knn_list_guided_k4, knn_list_epipolar_k4         the lists (max_distance = the median 4th distance of the window)
    knn_guided_p7_k8, knn_epipolar_p7_k8             7 pairs of the same two sets in one batched call
    knn_guided_7_singles_k8, knn_epipolar_7_singles_k8
and one chain (`chain`): match list -> verify -> epipolar rematch under the verified F -> verify, the rematch as the
k-NN list (k = 4) against the top-2 list.
Passes of every leg alternate; reported per leg: the median of the pass values and their range.  The bytes are checked
against sift_amd.cv.guided_knn / epipolar_knn / knn_records before anything is timed.

--parent-lib: a libsift_hip.so built from the parent commit.  match_device, match_knn_device (k = 4, 8),
match_guided_device and match_epipolar_device are then timed in child processes alternating between this build and
that one (SIFT_HIP_LIB), one interleaved pair per pass: their kernels are unchanged, so the ranges should overlap.
Written as measured."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sift_amd as sift  # noqa: E402
from match_epipolar_bench import INF, N, RADIUS, H, W, fundamental, setup  # noqa: E402
from match_knn_bench import stream_us, summary  # noqa: E402

MAX_ERROR = 1.95
P = 7
KS = (2, 4, 8)


class Legs:
    def __init__(self, q, t, dxy, F):
        import torch

        self.torch, self.q, self.t, self.F = torch, q, t, F
        self.qxy, self.txy = dxy[0].data_ptr(), dxy[1].data_ptr()
        self.m = sift.Matcher(N, N, max_pairs=P, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
        self.idx2, self.d2 = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32)
        self.idx, self.dk = torch.empty((P * N, 8), **i32), torch.empty((P * N, 8), **f32)
        self.recs, self.count = torch.empty((N * 8, 4), **i32), torch.empty(1, **i32)
        self.geo = torch.from_numpy(np.tile(np.asarray(F, np.float32).reshape(1, 9), (P, 1))).cuda()
        self.cap = 0.0

    def match_device(self):
        self.m.match_device(self.q, N, self.t, N, 0.8, False, self.idx2.data_ptr(), self.d2.data_ptr(), 0, self.st)

    def guided_top2(self):
        self.m.match_guided_device(self.q, N, self.t, N, self.qxy, self.txy, RADIUS, 2, 2, idx2_ptr=self.idx2.data_ptr(),
                                   d2_ptr=self.d2.data_ptr(), stream=self.st)

    def epipolar_top2(self):
        self.m.match_epipolar_device(self.q, N, self.t, N, self.qxy, self.txy, self.F, MAX_ERROR, INF, 2, 2,
                                     idx2_ptr=self.idx2.data_ptr(), d2_ptr=self.d2.data_ptr(), stream=self.st)

    def knn(self, k):
        self.m.match_knn_device(self.q, N, self.t, N, k, self.idx.data_ptr(), self.dk.data_ptr(), self.st)

    def knn_guided(self, k):
        self.m.match_knn_guided_device(self.q, N, self.t, N, self.qxy, self.txy, RADIUS, k, self.idx.data_ptr(),
                                       self.dk.data_ptr(), 2, 2, self.st)

    def knn_epipolar(self, k):
        self.m.match_knn_epipolar_device(self.q, N, self.t, N, self.qxy, self.txy, self.F, MAX_ERROR, k,
                                         self.idx.data_ptr(), self.dk.data_ptr(), INF, 2, 2, self.st)

    def list_guided(self):
        self.m.match_knn_list_guided_device(self.q, N, self.t, N, self.qxy, self.txy, RADIUS, 4, self.recs.data_ptr(),
                                            self.count.data_ptr(), self.cap, 2, 2, self.st)

    def list_epipolar(self):
        self.m.match_knn_list_epipolar_device(self.q, N, self.t, N, self.qxy, self.txy, self.F, MAX_ERROR, 4,
                                              self.recs.data_ptr(), self.count.data_ptr(), self.cap, INF, 2, 2, self.st)

    def batched_guided(self):
        self.m.match_knn_guided_batched([self.q] * P, [N] * P, [self.t] * P, [N] * P, [(self.qxy, self.txy)] * P, RADIUS,
                                        8, self.idx.data_ptr(), self.dk.data_ptr(), 2, 2, self.st)

    def batched_epipolar(self):
        self.m.match_knn_epipolar_batched([self.q] * P, [N] * P, [self.t] * P, [N] * P, [(self.qxy, self.txy)] * P,
                                          self.geo.data_ptr(), MAX_ERROR, 8, self.idx.data_ptr(), self.dk.data_ptr(), INF,
                                          36, 2, 2, self.st)

    def singles_guided(self):
        for _ in range(P):
            self.knn_guided(8)

    def singles_epipolar(self):
        for _ in range(P):
            self.knn_epipolar(8)

    def table(self, k, rows=N):
        self.torch.cuda.synchronize()
        n = rows * k
        return (self.idx.cpu().numpy().reshape(-1)[:n].reshape(rows, k).copy(),
                self.dk.cpu().numpy().reshape(-1)[:n].reshape(rows, k).copy())

    def records(self):
        self.torch.cuda.synchronize()
        n = int(self.count.cpu()[0])
        return self.recs.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n]

    def check(self, xy, host):
        """The bytes, before anything is timed."""
        from sift_amd import cv

        refs = {"guided": cv.guided_knn(host[0], host[1], xy[0], xy[1], RADIUS, 8),
                "epipolar": cv.epipolar_knn(host[0], host[1], xy[0], xy[1], self.F, MAX_ERROR, 8)}
        self.cap = float(np.median(np.sqrt(refs["guided"][1][:, 3][refs["guided"][0][:, 3] >= 0])))
        kept = {}
        for gate, fn, lst, bat in (("guided", self.knn_guided, self.list_guided, self.batched_guided),
                                   ("epipolar", self.knn_epipolar, self.list_epipolar, self.batched_epipolar)):
            ref = refs[gate]
            for k in KS:
                fn(k)
                gi, gd = self.table(k)
                if gi.tobytes() != np.ascontiguousarray(ref[0][:, :k]).tobytes() or \
                        gd.tobytes() != np.ascontiguousarray(ref[1][:, :k]).tobytes():
                    raise SystemExit(f"{gate} k = {k}: the table differs from the mirror: nothing to time")
            lst()
            exp = cv.knn_records(np.ascontiguousarray(ref[0][:, :4]), np.ascontiguousarray(ref[1][:, :4]), self.cap)
            if self.records().tobytes() != exp.tobytes() or not len(exp):
                raise SystemExit(f"{gate}: the list differs from cv.knn_records: nothing to time")
            kept[gate] = int(len(exp))
            bat()
            bi, bd = self.table(8, P * N)
            for p in range(P):
                if bi[p * N:(p + 1) * N].tobytes() != ref[0].tobytes() or bd[p * N:(p + 1) * N].tobytes() != ref[1].tobytes():
                    raise SystemExit(f"{gate}: batched pair {p} differs from the mirror: nothing to time")
        return {"list_kept": kept,
                "candidates_per_query_window": round(float(cv.gate_mask(xy[0], xy[1], RADIUS).sum(1).mean()), 2),
                "candidates_per_query_band": round(float(cv.epipolar_mask(xy[0], xy[1], self.F, MAX_ERROR).sum(1).mean()), 2)}


def measure(legs, xy, host, passes, calls):
    out = {"checks": legs.check(xy, host)}
    names = [("match_device", legs.match_device), ("guided_top2", legs.guided_top2), ("epipolar_top2", legs.epipolar_top2)]
    for k in KS:
        names += [(f"knn_k{k}", lambda k=k: legs.knn(k)), (f"knn_guided_k{k}", lambda k=k: legs.knn_guided(k)),
                  (f"knn_epipolar_k{k}", lambda k=k: legs.knn_epipolar(k))]
    names += [("knn_list_guided_k4", legs.list_guided), ("knn_list_epipolar_k4", legs.list_epipolar),
              ("knn_guided_p7_k8", legs.batched_guided), ("knn_epipolar_p7_k8", legs.batched_epipolar),
              ("knn_guided_7_singles_k8", legs.singles_guided), ("knn_epipolar_7_singles_k8", legs.singles_epipolar)]
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
    out["gated_over_ungated_knn"] = {f"{g}_k{k}": round(med(f"knn_{g}_k{k}") / med(f"knn_k{k}"), 3)
                                     for g in ("guided", "epipolar") for k in KS}
    out["knn_over_gated_top2"] = {f"{g}_k{k}": round(med(f"knn_{g}_k{k}") / med(f"{g}_top2"), 3)
                                  for g in ("guided", "epipolar") for k in KS}
    out["list_k4_minus_table_k4_us"] = {g: round(med(f"knn_list_{g}_k4") - med(f"knn_{g}_k4"), 2)
                                        for g in ("guided", "epipolar")}
    out["batched_over_7_singles"] = {g: round(med(f"knn_{g}_p7_k8") / med(f"knn_{g}_7_singles_k8"), 3)
                                     for g in ("guided", "epipolar")}
    return out


def chain(passes, calls):
    """match_list_device -> verify_device -> the epipolar rematch under the verified F read on the device ->
    verify_device on the rematch's list, on one stream without a read-back: the rematch as the k-NN list (k = 4,
    match_knn_list_epipolar_batched, P = 1) against the top-2 list (match_list_epipolar_batched).  The scene is
    tools/verify_bench.py's (1200 of 2000 rows planted under one F) with descriptors to match: a planted train row is
    its query row plus noise, and 300 other train rows are twins of planted queries (repetitive structure)."""
    import torch

    from sift_amd import cv
    from verify_bench import scene

    m0, q_xy, t_xy, planted = scene()
    rng = np.random.default_rng(5)
    q, t = rng.integers(0, 128, (N, 128)), rng.integers(0, 128, (N, 128))
    pl = m0[planted]
    t[pl["trainIdx"]] = np.clip(q[pl["queryIdx"]] + rng.integers(-3, 4, (len(pl), 128)), 0, 255)
    free = np.setdiff1d(np.arange(N), pl["trainIdx"])[:300]
    t[free] = np.clip(q[pl["queryIdx"][:300]] + rng.integers(-3, 4, (300, 128)), 0, 255)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float16)).view(np.int16)).cuda()  # noqa: E731
    dq, dt, dqxy, dtxy = up(q), up(t), torch.from_numpy(q_xy).cuda(), torch.from_numpy(t_xy).cuda()
    k, K, me = 4, 1024, 1.5
    mt, v = sift.Matcher(N, N, max_pairs=2, device=0), sift.Verifier(N * k, K, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    lst, cnt, res, res2 = torch.zeros((N, 4), **i32), torch.zeros(1, **i32), torch.zeros(13, **i32), torch.zeros(13, **i32)
    rl, rc = torch.zeros((N * k, 4), **i32), torch.zeros(1, **i32)
    inl, icnt = torch.zeros((N * k, 4), **i32), torch.zeros(1, **i32)
    mask = torch.zeros(N * k, dtype=torch.uint8, device="cuda")
    sets = ([dq.data_ptr()], [N], [dt.data_ptr()], [N], [(dqxy.data_ptr(), dtxy.data_ptr())])

    def run(knn):
        mt.match_list_device(dq.data_ptr(), N, dt.data_ptr(), N, lst.data_ptr(), cnt.data_ptr(), st)
        v.verify_device(lst.data_ptr(), cnt.data_ptr(), N, dqxy.data_ptr(), N, dtxy.data_ptr(), N, res.data_ptr(),
                        inl.data_ptr(), icnt.data_ptr(), mask.data_ptr(), me, K, 0, 2, 2, st)
        if knn:
            mt.match_knn_list_epipolar_batched(*sets, res.data_ptr(), me, k, rl.data_ptr(), rc.data_ptr(), 0.0, INF, 52, 2, 2,
                                               st)
        else:
            mt.match_list_epipolar_batched(*sets, res.data_ptr(), me, rl.data_ptr(), rc.data_ptr(), INF, 52, 2, 2, st)
        v.verify_device(rl.data_ptr(), rc.data_ptr(), N * k if knn else N, dqxy.data_ptr(), N, dtxy.data_ptr(), N,
                        res2.data_ptr(), inl.data_ptr(), icnt.data_ptr(), mask.data_ptr(), me, K, 0, 2, 2, st)

    checks = {}
    for name, knn in (("knn_k4", True), ("top2", False)):
        run(knn)
        torch.cuda.synchronize()
        r1 = res.cpu().numpy().view(sift.VERIFY_RESULT_DTYPE)[0]
        r2 = res2.cpu().numpy().view(sift.VERIFY_RESULT_DTYPE)[0]
        n = int(rc.cpu()[0])
        if r1["hypothesis"] < 0 or r2["hypothesis"] < 0:
            raise SystemExit(f"chain {name}: a verify pass found nothing: nothing to time")
        if knn:
            exp = cv.knn_records(*cv.epipolar_knn(q.astype(np.float32), t.astype(np.float32), q_xy, t_xy, r1["F"], me, k))
            if rl.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes() != exp.tobytes():
                raise SystemExit("chain: the k-NN rematch differs from the mirror: nothing to time")
        checks[name] = {"first_list": int(cnt.cpu()[0]), "first_inliers": int(r1["inliers"]), "rematch_list": n,
                        "second_inliers": int(r2["inliers"])}
    for _ in range(10):
        run(True), run(False)
    torch.cuda.synchronize()
    vals = {"knn_k4": [], "top2": []}
    for _ in range(passes):
        for name, knn in (("knn_k4", True), ("top2", False)):
            vals[name].append(stream_us(torch, lambda knn=knn: run(knn), calls))
    out = {"what": "us per chain, foreign fp16 buffers, K = 1024 hypotheses, max_error 1.5, k = 4", "checks": checks,
           "stream_us": {n: summary(x) for n, x in vals.items()}}
    out["knn_over_top2"] = round(out["stream_us"]["knn_k4"]["median"] / out["stream_us"]["top2"]["median"], 3)
    return out


CHILD_LEGS = ("match_device_detector", "match_device_foreign", "match_knn_device_k4", "match_knn_device_k8",
              "match_guided_device", "match_epipolar_device")


def child(calls):
    """The existing calls alone (this process's library: SIFT_HIP_LIB or the default build)."""
    import torch

    _det, bufs, (_rows, dxy), _xy, _host = setup()
    q, t = bufs["detector"]
    fq, ft = bufs["foreign"]
    F = fundamental()
    m = sift.Matcher(N, N, max_pairs=2, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    idx2, d2, match = torch.empty((N, 2), **i32), torch.empty((N, 2), **f32), torch.empty(N, **i32)
    idx, dk = torch.empty((N, 8), **i32), torch.empty((N, 8), **f32)
    qxy, txy = dxy[0].data_ptr(), dxy[1].data_ptr()
    out3 = dict(idx2_ptr=idx2.data_ptr(), d2_ptr=d2.data_ptr(), match_ptr=match.data_ptr(), stream=st)
    legs = {
        "match_device_detector": lambda: m.match_device(q, N, t, N, 0.8, False, idx2.data_ptr(), d2.data_ptr(),
                                                        match.data_ptr(), st),
        "match_device_foreign": lambda: m.match_device(fq, N, ft, N, 0.8, False, idx2.data_ptr(), d2.data_ptr(),
                                                       match.data_ptr(), st),
        "match_knn_device_k4": lambda: m.match_knn_device(q, N, t, N, 4, idx.data_ptr(), dk.data_ptr(), st),
        "match_knn_device_k8": lambda: m.match_knn_device(q, N, t, N, 8, idx.data_ptr(), dk.data_ptr(), st),
        "match_guided_device": lambda: m.match_guided_device(q, N, t, N, qxy, txy, RADIUS, 2, 2, **out3),
        "match_epipolar_device": lambda: m.match_epipolar_device(q, N, t, N, qxy, txy, F, MAX_ERROR, INF, 2, 2, **out3),
    }
    out = {"library": sift.version()}
    for name in CHILD_LEGS:
        fn = legs[name]
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
                               capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode or not line:
                raise SystemExit(f"child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
        print("pair", len(rows), json.dumps(pair), flush=True)
    out = {"pairs": rows}
    for leg in CHILD_LEGS:
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
    ap.add_argument("--chain-only", action="store_true", help="measure the chain alone and add it to the file at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_gated", "match_knn_gated_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("match_knn_gated_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    if a.chain_only:
        with open(a.out) as f:
            res = json.load(f)
        res["chain"] = chain(a.passes, max(a.calls // 4, 10))
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["chain"]))
        return
    _det, bufs, (_rows, dxy), xy, host = setup()
    F = fundamental()
    res = {"workload": f"{N} x {N} descriptors of two {W}x{H} synthetic frames (77, 78), numFeatures {N}; positions "
                       f"uniform in {W} x {H}; window radius {RADIUS:g}; F of a synthetic pair, max_error {MAX_ERROR}; "
                       f"stream_us: {a.calls} back-to-back calls between HIP events, per call ({max(a.calls // 4, 10)} "
                       f"for the 7-pair legs); {a.passes} interleaved passes, median of the pass values and their range",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "plan_splits": {"single": sift.Matcher.knn_plan(N, N, 1, 8), "p7": sift.Matcher.knn_plan(N, N, P, 8)},
           "not_measured": "occupancy and hardware counters; more than one GPU; the C++ surface",
           "routes": {}}
    for route in ("detector", "foreign"):
        q, t = bufs[route]
        res["routes"][route] = measure(Legs(q, t, dxy, F), xy, host, a.passes, a.calls)
        print(route, json.dumps(res["routes"][route]), flush=True)
    res["chain"] = chain(a.passes, max(a.calls // 4, 10))
    if a.parent_lib:
        res["existing_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
