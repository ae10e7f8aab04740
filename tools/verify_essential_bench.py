"""Cost of essential-matrix verification (Verifier.verify_essential_device: a fixed-budget 5-point RANSAC on the device,
ten model slots per sample) against the fundamental call of the same build at the same number of scored models, in the
same passes.

    python3 tools/verify_essential_bench.py [--passes 5] [--calls 200] [--parent-lib PATH]
                                            [--out profiles/essential/verify_essential_bench.json]

The list has the shape of tools/verify_bench.py's: 2000 records over shuffled position arrays in 1920 x 1200, 1200 of
them pairs of points seen by two cameras (focal length 1400, a rotation of 0.2 rad, a unit baseline, depths 4 .. 30
baselines; positions rounded to the quarter pixel) and 800 pairs of unrelated uniform positions.  Every result is
checked first: record, mask, list, samples, all 10 K models and counts must equal sift_amd.cv.ransac_essential byte for
byte.  Each leg is timed as `calls` back-to-back calls on one stream between two HIP events, per call; the passes of a
group's legs alternate, so clock and neighbour drift hit all alike; reported per leg: the median of the passes and
their range.

single    per K in {64, 256, 1024} samples: verify_essential_device (e); verify_device at 10 K hypotheses, the same
          number of scored models, where its 4096 limit allows (f: K = 64, 256); score_fundamental_device alone on the
          10 K models the essential call solved (s); and the essential call on the list's first five records (h): the
          gather, score and select launches are then near-empty, so this is the hypothesis kernel and three launch
          overheads -- the kernel was not isolated by a trace.
batched   P = 7, K = 256: one verify_essential_batched_device call against 7 single calls on the same stream and
          verifier.
--parent-lib  a libsift_hip.so built from the parent commit (tools/ab_build.sh): verify_device, verify_homography_device
          and recover_pose_device in child processes alternating between this build and that one (SIFT_HIP_LIB), one
          interleaved pair per pass; their kernels did not change and the ranges should overlap.
Not measured: occupancy or any other counter, a kernel trace (so no figure for the hypothesis kernel by itself), the
chain with the matcher or the pose call, K above 1024, anything beyond one GPU, the C++ surface."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_amd as sift  # noqa: E402
import verify_batched_bench as vbb  # noqa: E402  (stream_us)
import verify_bench as vb  # noqa: E402  (summary())
from sift_amd import cv  # noqa: E402

W, H, N, N_IN, MAX_ERROR = vb.W, vb.H, vb.N, vb.N_IN, vb.MAX_ERROR
KS = (64, 256, 1024)
K_BATCH, P = 256, 7
CAM = np.float32([1400.0, 1400.0, W / 2, H / 2])


def scene(seed=31):
    """(matches, q_xy, t_xy, planted): N records over (N, 2) float32 position arrays, N_IN of them pairs of one pose."""
    rng = np.random.default_rng(seed)
    a = np.array([0.3, 1.0, 0.2])
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(0.2) * Kx + (1 - np.cos(0.2)) * (Kx @ Kx)
    t = np.array([0.9, 0.1, 0.42])
    t = t / np.linalg.norm(t)
    Km = np.array([[CAM[0], 0, CAM[2]], [0, CAM[1], CAM[3]], [0, 0, 1]], np.float64)
    qa, ta = np.zeros((0, 2)), np.zeros((0, 2))
    while len(qa) < N_IN:
        X = np.stack([rng.uniform(-12, 12, 4 * N_IN), rng.uniform(-8, 8, 4 * N_IN), rng.uniform(4, 30, 4 * N_IN)], 1)
        Y = X @ R.T + t
        q, p = (X / X[:, 2:]) @ Km.T, (Y / Y[:, 2:]) @ Km.T
        ok = (Y[:, 2] > 1) & ((q[:, :2] >= 0) & (q[:, :2] < (W, H))).all(1) & ((p[:, :2] >= 0) & (p[:, :2] < (W, H))).all(1)
        qa, ta = np.r_[qa, q[ok, :2]], np.r_[ta, p[ok, :2]]
    q_xy, t_xy = rng.uniform(0, (W, H), (N, 2)), rng.uniform(0, (W, H), (N, 2))
    qrow, trow = rng.permutation(N), rng.permutation(N)
    q_xy[qrow[:N_IN]], t_xy[trow[:N_IN]] = qa[:N_IN], ta[:N_IN]
    order = rng.permutation(N)
    m = np.zeros(N, sift.DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["distance"] = qrow[order], trow[order], 1.0
    grid = lambda x: (np.rint(x * 4) / 4).astype(np.float32)  # noqa: E731
    return m, grid(q_xy), grid(t_xy), order < N_IN


def record(d):
    r = np.zeros(1, sift.VERIFY_RESULT_DTYPE)
    r["F"][0] = d["F"]
    for k in ("inliers", "hypothesis", "matches", "valid_hypotheses"):
        r[k][0] = d[k]
    return r


class Single:
    """The list on the device, a verifier that serves both models, and the outputs."""

    def __init__(self, max_pairs=1):
        import torch

        self.torch = torch
        self.m, self.q_xy, self.t_xy, self.planted = scene()
        self.dm = torch.from_numpy(self.m.view(np.int32).reshape(N, 4).copy()).cuda()
        self.dq, self.dt = torch.from_numpy(self.q_xy).cuda(), torch.from_numpy(self.t_xy).cuda()
        self.v = sift.Verifier(N * max_pairs, 4096, max_pairs, device=0, essential_samples=max(KS))
        self.st = torch.cuda.current_stream().cuda_stream
        i32 = dict(dtype=torch.int32, device="cuda")
        self.res, self.out, self.ints = torch.zeros(13, **i32), torch.zeros((N, 4), **i32), torch.zeros(2, **i32)
        self.mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(10 * max(KS), **i32)
        self.args = lambda n=N: (self.dm.data_ptr(), 0, n, self.dq.data_ptr(), N, self.dt.data_ptr(), N)
        self.Fs = {}

    def essential(self, K, n=N):
        self.v.verify_essential_device(*self.args(n), CAM, CAM, self.res.data_ptr(), self.out.data_ptr(),
                                       self.ints.data_ptr(), self.mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def fundamental(self, K):
        self.v.verify_device(*self.args(), self.res.data_ptr(), self.out.data_ptr(), self.ints.data_ptr(),
                             self.mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def score(self, K):
        self.v.score_device(*self.args(), self.Fs[K].data_ptr(), 10 * K, MAX_ERROR, self.counts.data_ptr(), 2, 2, self.st)

    def check(self, K):
        """The device's result against the numpy rule; keeps the models for the score leg."""
        self.essential(K)
        samples, F, valid, counts = self.v.essential_hypotheses()
        ref = cv.ransac_essential(self.m, self.q_xy, self.t_xy, CAM, CAM, MAX_ERROR, K, 0)
        n = int(self.ints.cpu()[0])
        listed = self.out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes()
        if (self.res.cpu().numpy().tobytes() != record(ref).tobytes() or n != ref["inliers"]
                or not np.array_equal(samples, ref["samples"]) or F.tobytes() != ref["Fs"].tobytes()
                or not np.array_equal(counts, ref["counts"]) or not np.array_equal(self.mask.cpu().numpy(), ref["mask"])
                or listed != ref["list"].tobytes()):
            raise SystemExit(f"K = {K}: the device result differs from the reference: nothing to time")
        if 10 * K <= 4096:
            self.Fs[K] = self.torch.from_numpy(F.copy()).cuda()
            self.score(K)
            self.torch.cuda.synchronize()
            got = self.counts.cpu().numpy()[:10 * K]  # score_device takes no valid flags: an all-zero model counts every record
            if not np.array_equal(got[ref["valid"]], ref["counts"][ref["valid"]]) or not (got[~ref["valid"]] == N).all():
                raise SystemExit(f"K = {K}: the score call differs from the reference: nothing to time")
        mask = ref["mask"] != 0
        out = {"slot": int(ref["hypothesis"]), "inliers": int(ref["inliers"]), "valid_slots": int(ref["valid_hypotheses"]),
               "planted_recovered": int((mask & self.planted).sum()), "outliers_admitted": int((mask & ~self.planted).sum())}
        if 10 * K <= 4096:
            f = cv.ransac_fundamental(self.m, self.q_xy, self.t_xy, MAX_ERROR, 10 * K, 0)
            fm = f["mask"] != 0
            out["fundamental_at_10K"] = {"inliers": int(f["inliers"]), "planted_recovered": int((fm & self.planted).sum()),
                                         "outliers_admitted": int((fm & ~self.planted).sum())}
        return out


def timed(torch, legs, passes):
    for _ in range(5):
        for _, fn, _c in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in legs}
    for _ in range(passes):
        for k, fn, c in legs:
            t[k].append(vbb.stream_us(torch, fn, c))
    return {k: vb.summary(v) for k, v in t.items()}


def single(passes, calls):
    import torch

    s = Single()
    out = {"results": {str(K): s.check(K) for K in KS}}
    legs = []
    for K in KS:
        legs += [(f"e{K}", lambda K=K: s.essential(K), calls), (f"h{K}", lambda K=K: s.essential(K, 5), calls)]
        if 10 * K <= 4096:
            legs += [(f"f{10 * K}", lambda K=K: s.fundamental(10 * K), calls), (f"s{10 * K}", lambda K=K: s.score(K), calls)]
    out["us_per_call"] = timed(torch, legs, passes)
    return out


def batched(passes, calls):
    import torch

    s = Single(P)
    i32 = dict(dtype=torch.int32, device="cuda")
    dm = s.dm.repeat(P, 1).contiguous()
    res, mask = torch.zeros(13 * P, **i32), torch.zeros(N * P, dtype=torch.uint8, device="cuda")
    res1, mask1 = torch.zeros(13 * P, **i32), torch.zeros(N * P, dtype=torch.uint8, device="cuda")
    pairs = [(s.dq.data_ptr(), N, s.dt.data_ptr(), N, N)] * P
    cams = np.tile(CAM, (P, 1))

    def one():
        s.v.verify_essential_batched_device(dm.data_ptr(), 0, pairs, cams, cams, res.data_ptr(), 0, 0, mask.data_ptr(),
                                            MAX_ERROR, K_BATCH, 0, 2, 2, s.st)

    def loop():
        for p in range(P):
            s.v.verify_essential_device(dm.data_ptr() + 16 * N * p, 0, N, s.dq.data_ptr(), N, s.dt.data_ptr(), N, CAM, CAM,
                                        res1.data_ptr() + 52 * p, 0, 0, mask1.data_ptr() + N * p, MAX_ERROR, K_BATCH, p, 2,
                                        2, s.st)

    one()
    loop()
    torch.cuda.synchronize()
    if res.cpu().numpy().tobytes() != res1.cpu().numpy().tobytes() or not torch.equal(mask, mask1):
        raise SystemExit("the batched call differs from the loop of single calls: nothing to time")
    t = timed(torch, [("batched", one, max(calls // P, 1)), ("loop", loop, max(calls // P, 1))], passes)
    return {"P": P, "K": K_BATCH, "us_per_call": t,
            "batched_wholly_below_loop": bool(t["batched"]["max"] < t["loop"]["min"])}


def child(calls):
    """verify_device, verify_homography_device and recover_pose_device alone (this process's library)."""
    import torch

    m, q_xy, t_xy, _ = scene()
    dm = torch.from_numpy(m.view(np.int32).reshape(N, 4).copy()).cuda()
    dq, dt = torch.from_numpy(q_xy).cuda(), torch.from_numpy(t_xy).cuda()
    v = sift.Verifier(N, 1024, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    res, resh, out, ints = torch.zeros(13, **i32), torch.zeros(13, **i32), torch.zeros((N, 4), **i32), torch.zeros(2, **i32)
    mask, pose = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(20, **i32)
    args = (dm.data_ptr(), 0, N, dq.data_ptr(), N, dt.data_ptr(), N)

    def f():
        v.verify_device(*args, res.data_ptr(), out.data_ptr(), ints.data_ptr(), mask.data_ptr(), MAX_ERROR, 1024, 0, 2, 2, st)

    def h():
        v.verify_homography_device(*args, resh.data_ptr(), out.data_ptr(), ints.data_ptr(), 0, MAX_ERROR, 1024, 0, 2, 2, st)

    def p():
        v.recover_pose_device(*args, res.data_ptr(), mask.data_ptr(), CAM, CAM, pose.data_ptr(), q_stride=2, t_stride=2,
                              stream=st)

    for _ in range(20):
        f(), h(), p()
    torch.cuda.synchronize()
    out_ = {"library": sift.version()}
    for k, fn in (("verify_device", f), ("verify_homography_device", h), ("recover_pose_device", p)):
        out_[k] = round(float(np.median([vbb.stream_us(torch, fn, calls) for _ in range(5)])), 2)
    print("CHILD " + json.dumps(out_), flush=True)


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
    for leg in ("verify_device", "verify_homography_device", "recover_pose_device"):
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": vb.summary(a), "parent_us": vb.summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential", "verify_essential_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    import torch

    out = {"library": sift.version(), "device": torch.cuda.get_device_name(0), "passes": a.passes, "calls": a.calls,
           "list": {"records": N, "planted": N_IN}, "single": single(a.passes, a.calls), "batched": batched(a.passes, a.calls)}
    if a.parent_lib:
        out["untouched_against_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    out["not_measured"] = ["counters", "a kernel trace: the hypothesis kernel by itself", "the chain with the matcher or the pose call",
                           "K above 1024", "more than one GPU", "the C++ surface"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "untouched_against_parent"}, indent=1))
    if a.parent_lib:
        print(json.dumps({k: v for k, v in out["untouched_against_parent"].items() if k != "pairs"}, indent=1))


if __name__ == "__main__":
    main()
