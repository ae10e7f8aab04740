"""Cost of the device plane pose recovery (Verifier.recover_pose_homography_device and its batched form:
cv::decomposeHomographyMat and the choice by visible points on the verifier's record, mask and list) on the homography
list of the verify benches: 2000 matches, 1200 pairs of a plane and 800 pairs of unrelated positions
(tools/verify_homography_bench.py), both cameras f = 1400 at the image centre.

    python3 tools/verify_pose_homography_bench.py [--passes 5] [--calls 100] [--parent-lib PATH]
                                                  [--out profiles/pose_homography/verify_pose_homography_bench.json]

Before anything is timed the device's plane pose record, candidates, in-front mask, points, in-front records and count
must equal the numpy rule sift_amd.cv.recover_pose_homography byte for byte (the single call; the batched call against
P single calls, and at P = 7 against the rule).  Each leg is timed as back-to-back repetitions on one stream between
two HIP events; the passes of a group's legs alternate, so clock and neighbour drift hit all alike; reported per leg:
the median of the passes and their range.

single      verify_homography_device -> refine_homography_device (K = 1024, rounds 1) once, then
            recover_pose_homography_device alone on the state they left: with every output (pose), and with the record
            alone (pose_record: no second pass, no candidates).  Beside them, in the same passes, the pose call from F of
            this build on tools/verify_bench.py's list of the same size (pose_from_F, pose_from_F_record): the same
            launch structure; both figures are reported and there is no bar between them.
batched     P = 7 and P = 56: one batched call against P single-pair calls on the same states.
chain       P = 7, K = 1024: verify_homography_batched_device -> refine_homography_batched_device ->
            recover_pose_homography_batched_device on one stream with no read-back, against the round trip it replaces:
            the same verify and refine calls, then the records, masks, lists and positions read back and
            sift_amd.cv.recover_pose_homography per pair on the host.
--parent-lib  a libsift_hip.so built from the parent commit (tools/ab_build.sh): verify_homography_device,
            refine_homography_device and recover_pose_device in child processes alternating between this build and that
            one, ranges expected to overlap: their kernels did not change.
Not measured: occupancy or any other counter, anything beyond one GPU, the C++ surface."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_amd as sift  # noqa: E402
import verify_batched_bench as vbb  # noqa: E402  (stream_us, PS)
import verify_bench as vb  # noqa: E402
import verify_pose_bench as vpb  # noqa: E402  (the pose call from F, for the comparison)
import verify_refit_bench as vrb  # noqa: E402  (Single, Refined, timed)
from sift_amd import cv  # noqa: E402

N, MAX_ERROR, K, CAM = vpb.N, vpb.MAX_ERROR, vpb.K, vpb.CAM


def pose_record(d):
    r = np.zeros(1, sift.PLANE_POSE_RESULT_DTYPE)
    r["R"][0], r["t"][0], r["in_front"], r["with_parallax"] = d["R"], d["t"], d["in_front"], d["with_parallax"]
    r["counts"][0], r["candidate"], r["fit"] = d["counts"], d["candidate"], d["fit"]
    r["normal"][0], r["distance"] = d["normal"], d["distance"]
    return r


def differs(got, ref):
    """The name of the first output of a plane pose call that is not the rule's, or None.  got: host arrays."""
    if got["pose"].tobytes() != pose_record(ref).tobytes():
        return "pose record"
    if got["cands"].tobytes() != ref["candidates"].tobytes():
        return "candidates"
    if not np.array_equal(got["front"], ref["mask"]):
        return "mask"
    if got["points"].view(np.uint32).tobytes() != ref["points"].view(np.uint32).tobytes():
        return "points"
    k = int(got["cnt"])
    if k != len(ref["list"]) or got["out"].view(sift.DMATCH_DTYPE).reshape(-1)[:k].tobytes() != ref["list"].tobytes():
        return "records"
    return None


class Single(vrb.Single):
    """The homography list verified and refined once, and the plane pose call's outputs."""

    def __init__(self):
        super().__init__("h")
        t = self.torch
        self.pose = t.zeros(24, dtype=t.int32, device="cuda")
        self.cands = t.zeros((4, 16), dtype=t.float32, device="cuda")
        self.front = t.zeros(N, dtype=t.uint8, device="cuda")
        self.points = t.zeros((N, 3), dtype=t.float32, device="cuda")
        self.pout, self.pcnt = t.zeros((N, 4), dtype=t.int32, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
        self.verify()
        self.refine(1)
        t.cuda.synchronize()

    def recover(self, full=True):
        self.v.recover_pose_homography_device(*self.args, self.res.data_ptr(), self.mask.data_ptr(), CAM, CAM,
                                              self.pose.data_ptr(), self.front.data_ptr() if full else 0,
                                              self.points.data_ptr() if full else 0, self.pout.data_ptr() if full else 0,
                                              self.pcnt.data_ptr() if full else 0, self.cands.data_ptr() if full else 0,
                                              q_stride=2, t_stride=2, stream=self.st)

    def check(self):
        self.recover()
        self.torch.cuda.synchronize()
        res = self.res.cpu().numpy().view(sift.HOMOGRAPHY_RESULT_DTYPE)[0]
        ref = cv.recover_pose_homography(self.m, self.q_xy, self.t_xy, res, self.mask.cpu().numpy(), CAM, CAM)
        got = dict(pose=self.pose.cpu().numpy(), cands=self.cands.cpu().numpy(), front=self.front.cpu().numpy(),
                   points=self.points.cpu().numpy(), out=self.pout.cpu().numpy(), cnt=self.pcnt.cpu().numpy()[0])
        bad = differs(got, ref)
        if bad:
            raise SystemExit(f"single: the device's {bad} differs from the rule: nothing to time")
        return {"inliers": int(res["inliers"]), "fit": int(ref["fit"]), "counts": [int(c) for c in ref["counts"]],
                "candidate": int(ref["candidate"]), "with_parallax": int(ref["with_parallax"]),
                "distance": float(ref["distance"]), "planted_in_front": int(((ref["mask"] != 0) & self.planted).sum())}


def single(passes, calls):
    import torch

    s = Single()
    checked = s.check()
    f = vpb.Single()
    f.check()
    us = vrb.timed(torch, [("pose", s.recover, calls), ("pose_record", lambda: s.recover(False), calls),
                           ("pose_from_F", f.recover, calls), ("pose_from_F_record", lambda: f.recover(False), calls)],
                   passes)
    out = {"checked": checked, "stream_us": us}
    print(f"single: {out['stream_us']['pose']['median']} us (from F {out['stream_us']['pose_from_F']['median']} us), {checked}",
          file=sys.stderr, flush=True)
    return out


class Posed(vrb.Refined):
    """tools/verify_refit_bench.py's homography batch, verified and refined, with the plane pose calls on two sets of
    outputs."""

    def __init__(self, P):
        super().__init__("h", P)
        t = self.torch
        i32 = dict(dtype=t.int32, device="cuda")
        self.cams = np.tile(CAM, (P, 1))
        self.pouts = [dict(pose=t.zeros((P, 24), **i32), cands=t.zeros((P, 4, 16), dtype=t.float32, device="cuda"),
                           front=t.zeros(P * N, dtype=t.uint8, device="cuda"),
                           points=t.zeros((P * N, 3), dtype=t.float32, device="cuda"), out=t.zeros((P * N, 4), **i32),
                           cnt=t.zeros(P, **i32)) for _ in range(2)]

    def prepare_pose(self):
        self.zero()
        self.batched(K)
        self.refine_batched(1, out=False)
        self.torch.cuda.synchronize()

    def pose_batched(self, full=True):
        o, p = self.outs[0], self.pouts[0]
        self.v.recover_pose_homography_batched_device(
            self.dm.data_ptr(), 0, self.pairs, o["res"].data_ptr(), o["mask"].data_ptr(), self.cams, self.cams,
            p["pose"].data_ptr(), p["front"].data_ptr() if full else 0, p["points"].data_ptr() if full else 0,
            p["out"].data_ptr() if full else 0, p["cnt"].data_ptr() if full else 0, p["cands"].data_ptr() if full else 0,
            q_stride=2, t_stride=2, stream=self.st)

    def pose_loop(self):
        o, p = self.outs[0], self.pouts[1]
        dm, res, mask = self.dm.data_ptr(), o["res"].data_ptr(), o["mask"].data_ptr()
        pose, cands, front, points, out, cnt = (p[k].data_ptr() for k in ("pose", "cands", "front", "points", "out", "cnt"))
        for i, (q, nq, t, nt, cap) in enumerate(self.pairs):
            self.v.recover_pose_homography_device(dm + 16 * N * i, 0, cap, q, nq, t, nt, res + 52 * i, mask + N * i, CAM, CAM,
                                                  pose + 96 * i, front + N * i, points + 12 * N * i, out + 16 * N * i,
                                                  cnt + 4 * i, cands + 256 * i, q_stride=2, t_stride=2, stream=self.st)

    def check_pose(self):
        self.prepare_pose()
        self.pose_batched()
        self.pose_loop()
        self.torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in self.pouts)
        for k in a:
            if a[k].tobytes() != b[k].tobytes():
                raise SystemExit(f"P = {self.P}: the batched plane pose call's {k} differs from the loop's: nothing to time")
        rec = a["pose"].view(sift.PLANE_POSE_RESULT_DTYPE).reshape(-1)
        if self.P == min(vbb.PS):
            res = self.outs[0]["res"].cpu().numpy().view(sift.HOMOGRAPHY_RESULT_DTYPE).reshape(-1)
            masks = self.outs[0]["mask"].cpu().numpy().reshape(self.P, N)
            for p in range(self.P):
                ref = cv.recover_pose_homography(self.lists[p], self.q_xy, self.t_xy, res[p], masks[p], CAM, CAM)
                got = dict(pose=a["pose"][p], cands=a["cands"][p], front=a["front"][N * p: N * (p + 1)],
                           points=a["points"][N * p: N * (p + 1)], out=a["out"][N * p: N * (p + 1)], cnt=a["cnt"][p])
                bad = differs(got, ref)
                if bad:
                    raise SystemExit(f"pair {p}: the device's {bad} differs from the rule: nothing to time")
        return {"poses": int((rec["candidate"] >= 0).sum()), "in_front_min": int(rec["in_front"].min()),
                "in_front_max": int(rec["in_front"].max())}


def batched(passes, calls):
    import torch

    out = {}
    for P in vbb.PS:
        b = Posed(P)
        checked = b.check_pose()
        us = vrb.timed(torch, [("b", b.pose_batched, calls), ("l", b.pose_loop, max(calls // 5, 4))], passes)
        out[f"P{P}"] = {"checked": checked, "stream_us": us,
                        "loop_over_batched": round(us["l"]["median"] / us["b"]["median"], 2),
                        "batched_wholly_below_loop": bool(us["b"]["max"] < us["l"]["min"])}
        print(f"batched P = {P}: {out[f'P{P}']}", file=sys.stderr, flush=True)
        del b
    return out


def chain(passes, calls):
    """verify -> refine -> pose on the device against verify -> refine -> read-back -> the rule per pair on the host."""
    import torch

    b = Posed(min(vbb.PS))
    b.check_pose()
    P = b.P
    host_s = []

    def device():
        b.batched(K)
        b.refine_batched(1, out=False)
        b.pose_batched()

    def round_trip():
        b.batched(K)
        b.refine_batched(1, out=False)
        res = b.outs[0]["res"].cpu().numpy().view(sift.HOMOGRAPHY_RESULT_DTYPE).reshape(-1)  # synchronises
        masks = b.outs[0]["mask"].cpu().numpy().reshape(P, N)
        lists = b.dm.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(P, N)
        xy = [(q.cpu().numpy(), t.cpu().numpy()) for q, t in zip(b.dq, b.dt)]
        t0 = time.perf_counter()
        for p in range(P):
            cv.recover_pose_homography(lists[p], xy[p][0], xy[p][1], res[p], masks[p], CAM, CAM)
        host_s.append(time.perf_counter() - t0)

    def wall_us(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e6

    for _ in range(3):
        device()
        round_trip()
    host_s.clear()
    t = {"device_chain": [], "round_trip": []}
    for _ in range(passes):
        t["device_chain"].append(wall_us(device, calls))
        t["round_trip"].append(wall_us(round_trip, max(calls // 10, 4)))
    us = {k: vb.summary(v) for k, v in t.items()}
    out = {"pairs": P, "hypotheses": K, "wall_us": us,
           "host_recover_pose_homography_us_per_call": round(float(np.median(host_s)) * 1e6, 1),
           "round_trip_over_device_chain": round(us["round_trip"]["median"] / us["device_chain"]["median"], 2)}
    print(f"chain: {out}", file=sys.stderr, flush=True)
    return out


def child(calls):
    """The existing single-pair calls alone (this process's library): verify_homography_device,
    refine_homography_device (K = 1024) and recover_pose_device."""
    import torch

    s = vrb.Single("h")
    s.verify()
    s.refine(1)
    f = vpb.Single()
    torch.cuda.synchronize()
    legs = [("verify_homography_device", s.verify), ("refine_homography_device", lambda: s.refine(1)),
            ("recover_pose_device", f.recover)]
    for _ in range(20):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(5):
        for k, fn in legs:
            t[k].append(vbb.stream_us(torch, fn, calls))
    out = {"library": sift.version()}
    out.update({k: round(float(np.median(x)), 2) for k, x in t.items()})
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
                raise SystemExit(f"single-pair child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
            print(f"child {name}: {line[-1][6:]}", file=sys.stderr, flush=True)
        rows.append(pair)
    out = {"pairs": rows}
    for leg in [k for k in rows[0]["this"] if k != "library"]:
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": vb.summary(a), "parent_us": vb.summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_homography", "verify_pose_homography_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_pose_homography_bench needs a GPU: nothing is measured without one")
    if a.child:
        return child(a.calls)
    res = {"workload": f"{N} matches per list (the plane of tools/verify_homography_bench.py), cameras {CAM.tolist()}, "
                       f"K = {K}, max_error {MAX_ERROR}, refit rounds 1, default pose thresholds; stream_us: back-to-back "
                       f"repetitions between HIP events, per repetition; wall_us: host clock around synchronised repetitions",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "not_measured": "occupancy or any other hardware counter; more than one GPU; the C++ surface"}
    res["single"] = single(a.passes, a.calls)
    res["batched_vs_loop"] = batched(a.passes, a.calls)
    res["chain"] = chain(a.passes, a.calls)
    if a.parent_lib:
        res["existing_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, max(a.calls, 200))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
