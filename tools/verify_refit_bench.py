"""Cost and effect of the device refit (Verifier.refine_device / refine_homography_device and their batched forms:
the least-squares model on the inliers, rescored and kept when it counts at least as many) on the lists of the verify
benches: 2000 matches, 1200 true pairs of a two-camera scene (tools/verify_bench.py; a plane for the homography,
tools/verify_homography_bench.py) and 800 pairs of unrelated positions.

    python3 tools/verify_refit_bench.py [--passes 5] [--calls 100] [--parent-lib PATH]
                                        [--out profiles/refit/verify_refit_bench.json]

Before anything is timed the device's refined record, mask, inlier records, count and accepted rounds must equal the
numpy rule sift_amd.cv.refine_fundamental / refine_homography byte for byte (single calls at rounds 1 and 2; the
batched call against P single calls, and at P = 7 against the rule).  Each leg is timed as back-to-back repetitions on
one stream between two HIP events; the passes of a group's legs alternate, so clock and neighbour drift hit all alike;
reported per leg: the median of the passes and their range.

single      per model, K = 1024: verify_device alone (v), verify_device followed by refine_device at rounds 1 and 2
            (vr1, vr2: the refit starts from the verify call's state every time), and refine_device alone on the state it
            left (r1, r2: the same kernels on a converged model).  The refit's cost is vr - v.
quality     numbers only: the inlier count and the RMS Sampson distance / transfer error (float64, pixels) of the 1200
            true pairs under the model before and after the refit.
batched     P = 7 and P = 56, rounds 1: one batched refine call against P single-pair refine calls on the same states.
chain       P = 7, K = 1024: verify_batched_device -> refine_batched_device (rounds 1) on one stream with no read-back,
            against the round trip it replaces: verify_batched_device, the results, counts and inlier records read
            back, sift_amd.cv.fundamental_lstsq / homography_lstsq per pair on the host, nine floats per pair uploaded.
            match_list_batched before and the guided rematch after are the same calls on both sides and are left out.
--parent-lib  a libsift_hip.so built from the parent commit (tools/ab_build.sh): verify_device, score_device and
            verify_homography_device in child processes alternating between this build and that one
            (tools/verify_batched_bench.py's legs), ranges expected to overlap: their kernels did not change.
Not measured: occupancy or any other counter, anything beyond one GPU, the C++ surface."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_amd as sift  # noqa: E402
import verify_batched_bench as vbb  # noqa: E402  (Batch, stream_us, parent_pairs)
import verify_bench as vb  # noqa: E402
import verify_homography_bench as vhb  # noqa: E402
from sift_amd import cv  # noqa: E402

N, MAX_ERROR, K = vb.N, vb.MAX_ERROR, 1024
FIELD = {"f": "F", "h": "H"}
DTYPE = {"f": sift.VERIFY_RESULT_DTYPE, "h": sift.HOMOGRAPHY_RESULT_DTYPE}
RULES = {"f": (cv.ransac_fundamental, cv.refine_fundamental, cv.fundamental_lstsq),
         "h": (cv.ransac_homography, cv.refine_homography, cv.homography_lstsq)}


def record(model, d):
    r = np.zeros(1, DTYPE[model])
    r[FIELD[model]][0] = d[FIELD[model]]
    for k in ("inliers", "hypothesis", "matches", "valid_hypotheses"):
        r[k][0] = d[k]
    return r


def rms_error(model, M, pts):
    """The RMS Sampson distance (f) or forward transfer error (h) of float64 points (n, 4) under M, in pixels."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    q, t = np.c_[pts[:, :2], np.ones(len(pts))], np.c_[pts[:, 2:], np.ones(len(pts))]
    if model == "f":
        l, lt = q @ M.T, t @ M
        r = (t * l).sum(1)
        d2 = r * r / (l[:, 0] ** 2 + l[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)
    else:
        p = q @ M.T
        d2 = ((p[:, :2] / p[:, 2:] - pts[:, 2:]) ** 2).sum(1)
    return round(float(np.sqrt(d2.mean())), 4)


class Single:
    """One list of a model on the device, its verifier and outputs."""

    def __init__(self, model):
        import torch

        self.torch, self.model = torch, model
        self.m, self.q_xy, self.t_xy, self.planted = vhb.plane_scene() if model == "h" else vb.scene()
        self.dm = torch.from_numpy(self.m.view(np.int32).reshape(N, 4).copy()).cuda()
        self.dq, self.dt = torch.from_numpy(self.q_xy).cuda(), torch.from_numpy(self.t_xy).cuda()
        self.v = sift.Verifier(N, K, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        i32 = dict(dtype=torch.int32, device="cuda")
        self.res, self.out, self.ints = torch.zeros(13, **i32), torch.zeros((N, 4), **i32), torch.zeros(2, **i32)
        self.mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.args = (self.dm.data_ptr(), 0, N, self.dq.data_ptr(), N, self.dt.data_ptr(), N)

    def verify(self):
        fn = self.v.verify_homography_device if self.model == "h" else self.v.verify_device
        fn(*self.args, self.res.data_ptr(), 0, 0, self.mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def refine(self, rounds):
        fn = self.v.refine_homography_device if self.model == "h" else self.v.refine_device
        fn(*self.args, self.res.data_ptr(), self.mask.data_ptr(), self.out.data_ptr(), self.ints.data_ptr(),
           self.ints.data_ptr() + 4, MAX_ERROR, rounds, 2, 2, self.st)

    def check(self):
        """verify -> refine at rounds 1 and 2 against the rule; the quality numbers."""
        ransac, refine, _ = RULES[self.model]
        ref0 = ransac(self.m, self.q_xy, self.t_xy, MAX_ERROR, K, 0)
        pts = cv._match_points(self.m, self.q_xy, self.t_xy).astype(np.float64)[self.planted]
        f = FIELD[self.model]
        out = {"before": {"inliers": int(ref0["inliers"]), "true_pairs_rms_px": rms_error(self.model, ref0[f], pts)}}
        for rounds in (1, 2):
            self.verify()
            self.refine(rounds)
            self.torch.cuda.synchronize()
            ref = refine(self.m, self.q_xy, self.t_xy, ref0, MAX_ERROR, rounds)
            ints = self.ints.cpu().numpy()
            n = int(ints[0])
            if (self.res.cpu().numpy().tobytes() != record(self.model, ref).tobytes() or int(ints[1]) != ref["accepted"]
                    or not np.array_equal(self.mask.cpu().numpy(), ref["mask"]) or n != len(ref["list"])
                    or self.out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes() != ref["list"].tobytes()):
                raise SystemExit(f"{self.model} rounds = {rounds}: the device refit differs from the rule: nothing to time")
            mask = ref["mask"] != 0
            out[f"rounds_{rounds}"] = {"inliers": int(ref["inliers"]), "accepted": int(ref["accepted"]),
                                       "true_pairs_rms_px": rms_error(self.model, ref[f], pts),
                                       "planted_recovered": int((mask & self.planted).sum()),
                                       "outliers_admitted": int((mask & ~self.planted).sum())}
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

    out = {}
    for model in "fh":
        s = Single(model)
        quality = s.check()

        def vr(rounds, s=s):
            s.verify()
            s.refine(rounds)

        legs = [("v", s.verify, calls), ("vr1", lambda: vr(1), calls), ("vr2", lambda: vr(2), calls),
                ("r1", lambda s=s: s.refine(1), calls), ("r2", lambda s=s: s.refine(2), calls)]
        us = timed(torch, legs, passes)
        out[model] = {"quality": quality, "stream_us": us,
                      "refit_cost_us": {"rounds_1": round(us["vr1"]["median"] - us["v"]["median"], 2),
                                        "rounds_2": round(us["vr2"]["median"] - us["v"]["median"], 2)},
                      "refit_over_verify": {"rounds_1": round(us["r1"]["median"] / us["v"]["median"], 3),
                                            "rounds_2": round(us["r2"]["median"] / us["v"]["median"], 3)}}
        print(f"single {model}: {out[model]['refit_cost_us']} {quality}", file=sys.stderr, flush=True)
    return out


class Refined(vbb.Batch):
    """tools/verify_batched_bench.py's batch, verified, with the refine calls on its two sets of outputs."""

    def __init__(self, model, P):
        super().__init__(model, P)
        i32 = dict(dtype=self.torch.int32, device="cuda")
        for o in self.outs:
            o["acc"] = self.torch.zeros(P, **i32)

    def prepare(self):
        self.zero()
        self.batched(K)
        self.loop(K)
        self.torch.cuda.synchronize()
        self.verified = {k: t.cpu().numpy().copy() for k, t in self.outs[0].items()}

    def refine_batched(self, rounds=1, out=True):
        o = self.outs[0]
        fn = self.v.refine_homography_batched_device if self.model == "h" else self.v.refine_batched_device
        fn(self.dm.data_ptr(), 0, self.pairs, o["res"].data_ptr(), o["mask"].data_ptr(), o["out"].data_ptr() if out else 0,
           o["cnt"].data_ptr() if out else 0, o["acc"].data_ptr(), MAX_ERROR, rounds, 2, 2, self.st)

    def refine_loop(self, rounds=1):
        o = self.outs[1]
        fn = self.v.refine_homography_device if self.model == "h" else self.v.refine_device
        dm, res, out, cnt, mask, acc = (t.data_ptr() for t in (self.dm, o["res"], o["out"], o["cnt"], o["mask"], o["acc"]))
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            fn(dm + 16 * N * p, 0, cap, q, nq, t, nt, res + 52 * p, mask + N * p, out + 16 * N * p, cnt + 4 * p, acc + 4 * p,
               MAX_ERROR, rounds, 2, 2, self.st)

    def check(self):
        self.prepare()
        self.refine_batched()
        self.refine_loop()
        self.torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in self.outs)
        for k in a:
            if a[k].tobytes() != b[k].tobytes():
                raise SystemExit(f"{self.model} P = {self.P}: the batched refit's {k} differs from the loop's: nothing to time")
        rec = a["res"].view(DTYPE[self.model]).reshape(-1)
        if self.P == min(vbb.PS):
            ransac, refine, _ = RULES[self.model]
            for p in range(self.P):
                ref = refine(self.lists[p], self.q_xy, self.t_xy, ransac(self.lists[p], self.q_xy, self.t_xy, MAX_ERROR, K, p),
                             MAX_ERROR, 1)
                if (rec[p:p + 1].tobytes() != record(self.model, ref).tobytes() or a["acc"][p] != ref["accepted"]
                        or not np.array_equal(a["mask"][N * p: N * (p + 1)], ref["mask"])):
                    raise SystemExit(f"{self.model} pair {p}: the batched refit differs from the rule: nothing to time")
        return {"accepted_pairs": int((a["acc"] > 0).sum()), "inliers_min": int(rec["inliers"].min()),
                "inliers_max": int(rec["inliers"].max())}


def batched(passes, calls):
    import torch

    out = {}
    for model in "fh":
        for P in vbb.PS:
            b = Refined(model, P)
            checked = b.check()
            us = timed(torch, [("b", b.refine_batched, calls), ("l", b.refine_loop, max(calls // 5, 4))], passes)
            out[f"{model}_P{P}"] = {"checked": checked, "stream_us": us,
                                    "loop_over_batched": round(us["l"]["median"] / us["b"]["median"], 2),
                                    "batched_wholly_below_loop": bool(us["b"]["max"] < us["l"]["min"])}
            print(f"batched {model} P = {P}: {out[f'{model}_P{P}']['loop_over_batched']}", file=sys.stderr, flush=True)
            del b
    return out


def chain(passes, calls):
    """verify -> refine on the device against verify -> read-back -> host least squares -> upload, P = 7."""
    import torch

    out = {}
    for model in "fh":
        b = Refined(model, min(vbb.PS))
        b.check()
        P, lstsq = b.P, RULES[model][2]
        geometry = torch.zeros((P, 9), dtype=torch.float32, device="cuda")
        pts = [cv._match_points(b.lists[p], b.q_xy, b.t_xy) for p in range(P)]
        host_s = []

        def device():
            b.batched(K)
            b.refine_batched(1, out=False)

        def round_trip():
            b.batched(K)
            res = b.outs[0]["res"].cpu().numpy().view(DTYPE[model]).reshape(-1)  # synchronises
            masks = b.outs[0]["mask"].cpu().numpy().reshape(P, N)
            t0 = time.perf_counter()
            fit = np.zeros((P, 9), np.float32)
            for p in range(P):
                inl = masks[p] != 0
                if res[p]["hypothesis"] >= 0 and inl.sum() >= 8:
                    M = lstsq(pts[p][inl, :2], pts[p][inl, 2:])
                    fit[p] = (M / np.linalg.norm(M)).reshape(9)
            host_s.append(time.perf_counter() - t0)
            geometry.copy_(torch.from_numpy(fit))

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
        out[model] = {"pairs": P, "hypotheses": K, "wall_us": us,
                      "host_least_squares_us_per_call": round(float(np.median(host_s)) * 1e6, 1),
                      "round_trip_over_device_chain": round(us["round_trip"]["median"] / us["device_chain"]["median"], 2)}
        print(f"chain {model}: {out[model]}", file=sys.stderr, flush=True)
        del b
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "verify_refit_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_refit_bench needs a GPU: nothing is measured without one")
    res = {"workload": f"{N} matches per list (the scenes of tools/verify_bench.py and tools/verify_homography_bench.py), "
                       f"K = {K}, max_error {MAX_ERROR}, seed 0 (pair p: seed p); stream_us: back-to-back repetitions "
                       f"between HIP events, per repetition; wall_us: host clock around synchronised repetitions",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "not_measured": "occupancy or any other hardware counter; more than one GPU; the C++ surface; the matcher calls "
                           "around the chain (identical on both of its sides)"}
    res["single"] = single(a.passes, a.calls)
    res["batched_vs_loop"] = batched(a.passes, a.calls)
    res["chain"] = chain(a.passes, a.calls)
    if a.parent_lib:
        res["single_pair_calls_vs_parent"] = vbb.parent_pairs(os.path.abspath(a.parent_lib), a.passes, max(a.calls, 200))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
