"""Cost of batched guided matching (Matcher.match_guided_batched / match_epipolar_batched and their list forms: all P
pairs under a gate in one pass) against the same P pairs through P single-pair calls, at the shapes of the all-pairs
exchange: P = 7 (one GPU's share of 8 sets) and P = 28 (all unordered pairs), 2000 x 2000 rows per pair.

    python3 tools/match_guided_batched_bench.py [--passes 5] [--calls 100] [--parent-lib PATH]
                                                [--out profiles/guided_batched/match_guided_batched_bench.json]

The sets are the descriptors of 8 synthetic frames (1920 x 1200, up to 2000 rows each) in foreign fp16 buffers, the
positions uniform in 1920 x 1200 (tools/match_epipolar_bench.py's workload); the window has radius 50, the band the
max_error that gives a query about the window's candidate count (8.5), pair p's F is that tool's F times a constant
of its own.  Legs, per gate (w: window, e: epipolar) and P:
    bt  one batched top-2 call              lt  P single-pair top-2 calls back to back
    bl  one batched cross-checked list      ll  P single-pair list calls back to back
on the same stream and the same matcher (max_pairs = 2 P: both directions of a list in one pass).  Before anything is
timed the batched outputs must equal the loop's byte for byte (records modulo imgIdx).  Each leg is timed as `calls`
(loops: calls / 5) back-to-back repetitions between two HIP events; passes of the legs alternate, so clock and
neighbour drift hit all alike; reported per leg: the median of the passes and their range, loop over batched as the
ratio of the medians, and whether the batched call's whole range lies below the loop's.

The chains, P = 7, K = 1024, on one stream:
    h   match_list_batched -> verify_homography_batched_device -> project_homography_batched_device ->
        match_list_guided_batched                  against the same with 7 single projections + 7 single guided lists
    f   match_list_batched -> verify_batched_device -> match_list_epipolar_batched(geometry = the result records)
                                                   against the same with the 7-record read-back + 7 single epipolar lists
(the positions are uniform, so the geometry found is meaningless; the work is the same).

--parent-lib: a libsift_hip.so built from the parent commit (tools/ab_build.sh).  The single-pair calls match_device,
match_guided_device and match_epipolar_device are then timed in child processes alternating between this build and
that one (SIFT_HIP_LIB), one interleaved pair per pass: their kernels are untouched, so the ranges should overlap.

Not measured here: the occupancy of the new kernels, and anything beyond one GPU."""
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
import match_epipolar_bench as eb  # noqa: E402  (F, band_for, summary)

W, H, N, RADIUS = eb.W, eb.H, eb.N, eb.RADIUS
INF = float("inf")
PS = (7, 28)
SCALES = (1.0, 3.0, 0.7, 5.0, 1.3, 11.0, 0.9)


def stream_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def setup():
    """8 sets of up to N rows (foreign fp16 buffers), their counts, and uniform positions (host and device)."""
    import torch

    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=N), device=0)
    det.gpuWarmUpAndAllocate()
    sets, ns = [], []
    for i in range(8):
        det.detectAndCompute(sift.synth_frame(77 + i, W, H))
        n = min(det.total_size, N)
        if n < N // 2:
            raise SystemExit(f"frame {77 + i} gave {det.total_size} keypoints: not the workload")
        d = torch.zeros((N, 128), dtype=torch.float16, device="cuda")
        sift._check(sift.lib().sift_hip_memcpy_d2d(d.data_ptr(), det.device_descriptor.data(), 256 * n, None), "d2d")
        sets.append(d)
        ns.append(n)
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    xy = [(rng.random((N, 2)) * (W, H)).astype(np.float32) for _ in range(8)]
    dxy = [torch.from_numpy(a).cuda() for a in xy]
    return sets, ns, xy, dxy


class Batch:
    def __init__(self, torch, world, P, max_error):
        sets, ns, xy, dxy = world
        self.torch, self.P, self.max_error = torch, P, max_error
        ij = [(0, j) for j in range(1, 8)] if P == 7 else [(i, j) for i in range(8) for j in range(i + 1, 8)]
        assert len(ij) == P
        self.q, self.nq = [sets[i].data_ptr() for i, _ in ij], [ns[i] for i, _ in ij]
        self.t, self.nt = [sets[j].data_ptr() for _, j in ij], [ns[j] for _, j in ij]
        self.pos = [(dxy[i].data_ptr(), dxy[j].data_ptr()) for i, j in ij]
        self.F = np.stack([eb.fundamental() * np.float32(SCALES[p % len(SCALES)]) for p in range(P)]).astype(np.float32)
        self.dF = torch.from_numpy(self.F.reshape(P, 9)).cuda()
        self.m = sift.Matcher(N, N, max_pairs=2 * P, device=0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.row0 = np.concatenate([[0], np.cumsum(self.nq)]).astype(int)
        rows = int(self.row0[-1])
        i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
        self.o = [dict(idx2=torch.zeros((rows, 2), **i32), d2=torch.zeros((rows, 2), **f32), match=torch.zeros(rows, **i32),
                       recs=torch.zeros((rows, 4), **i32), cnt=torch.zeros(P, **i32)) for _ in range(2)]

    def bt(self, gate):
        o = self.o[0]
        a = (self.q, self.nq, self.t, self.nt, self.pos)
        out = (0.8, False, o["idx2"].data_ptr(), o["d2"].data_ptr(), o["match"].data_ptr(), self.st)
        if gate == "w":
            self.m.match_guided_batched(*a, RADIUS, 2, 2, *out)
        else:
            self.m.match_epipolar_batched(*a, self.dF.data_ptr(), self.max_error, INF, 36, 2, 2, *out)

    def lt(self, gate):
        o = self.o[1]
        for p in range(self.P):
            r = int(self.row0[p])
            a = (self.q[p], self.nq[p], self.t[p], self.nt[p], self.pos[p][0], self.pos[p][1])
            out = (2, 2, 0.8, False, o["idx2"].data_ptr() + 8 * r, o["d2"].data_ptr() + 8 * r, o["match"].data_ptr() + 4 * r,
                   self.st)
            if gate == "w":
                self.m.match_guided_device(*a, RADIUS, *out)
            else:
                self.m.match_epipolar_device(*a, self.F[p], self.max_error, INF, *out)

    def bl(self, gate):
        o = self.o[0]
        a = (self.q, self.nq, self.t, self.nt, self.pos)
        if gate == "w":
            self.m.match_list_guided_batched(*a, RADIUS, o["recs"].data_ptr(), o["cnt"].data_ptr(), 2, 2, self.st)
        else:
            self.m.match_list_epipolar_batched(*a, self.dF.data_ptr(), self.max_error, o["recs"].data_ptr(),
                                               o["cnt"].data_ptr(), INF, 36, 2, 2, self.st)

    def ll(self, gate):
        o = self.o[1]
        for p in range(self.P):
            r = int(self.row0[p])
            a = (self.q[p], self.nq[p], self.t[p], self.nt[p], self.pos[p][0], self.pos[p][1])
            out = (o["recs"].data_ptr() + 16 * r, o["cnt"].data_ptr() + 4 * p)
            if gate == "w":
                self.m.match_list_guided_device(*a, RADIUS, *out, 2, 2, self.st)
            else:
                self.m.match_list_epipolar_device(*a, self.F[p], self.max_error, *out, INF, 2, 2, self.st)

    def check(self, gate):
        for o in self.o:
            for t in o.values():
                t.zero_()
        self.bt(gate), self.lt(gate), self.bl(gate), self.ll(gate)
        self.torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in self.o)
        for k in ("idx2", "d2", "match", "cnt"):
            if a[k].tobytes() != b[k].tobytes():
                raise SystemExit(f"{gate} P = {self.P}: the batched call's {k} differs from the loop's: nothing to time")
        ra, rb = (x["recs"].copy().view(sift.DMATCH_DTYPE).reshape(-1) for x in (a, b))
        for p in range(self.P):
            n, r = int(a["cnt"][p]), int(self.row0[p])
            x, y = ra[r:r + n].copy(), rb[r:r + n].copy()
            if not np.all(x["imgIdx"] == p) or not np.all(y["imgIdx"] == 0):
                raise SystemExit(f"{gate} pair {p}: imgIdx")
            x["imgIdx"] = 0
            if x.tobytes() != y.tobytes():
                raise SystemExit(f"{gate} P = {self.P} pair {p}: the batched list differs from the loop's: nothing to time")
        return {"kept": a["cnt"].tolist(), "queries_with_a_candidate": int((a["idx2"][:, 0] >= 0).sum())}


def timed(torch, legs, passes):
    for _ in range(3):
        for _, fn, _c in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in legs}
    for _ in range(passes):
        for k, fn, c in legs:
            t[k].append(stream_us(torch, fn, c))
    return {k: eb.summary(v) for k, v in t.items()}


def measure(torch, world, max_error, passes, calls):
    out = {}
    for P in PS:
        b = Batch(torch, world, P, max_error)
        for gate in "we":
            checked = b.check(gate)
            few = max(calls // 5, 4)
            legs = [("bt", lambda: b.bt(gate), calls), ("lt", lambda: b.lt(gate), few), ("bl", lambda: b.bl(gate), calls),
                    ("ll", lambda: b.ll(gate), few)]
            leg = {"checked": checked, "stream_us": timed(torch, legs, passes)}
            for x, y, name in (("bt", "lt", "top2"), ("bl", "ll", "list")):
                bb, lo = leg["stream_us"][x], leg["stream_us"][y]
                leg[name] = {"loop_over_batched": round(lo["median"] / bb["median"], 2),
                             "batched_us_per_pair": round(bb["median"] / P, 2), "loop_us_per_pair": round(lo["median"] / P, 2),
                             "batched_wholly_below_loop": bool(bb["max"] < lo["min"])}
            out[f"{gate}_P{P}"] = leg
            print(f"measured {gate} P = {P}: {leg['top2']} {leg['list']}", file=sys.stderr, flush=True)
        del b
    return out


def chains(torch, world, max_error, passes, calls):
    from sift_amd import cv

    sets, ns, _xy, dxy = world
    P, K = 7, 1024
    qp, nqs = [sets[0].data_ptr()] * P, [ns[0]] * P
    tp, nts = [sets[j].data_ptr() for j in range(1, 8)], ns[1:]
    rows = sum(nqs)
    row0 = np.concatenate([[0], np.cumsum(nqs)]).astype(int)
    m, v = sift.Matcher(N, N, max_pairs=2 * P, device=0), sift.Verifier(rows, K, P, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    lst, cnt, res = torch.zeros((rows, 4), **i32), torch.zeros(P, **i32), torch.zeros((P, 13), **i32)
    proj = [torch.zeros((nqs[p], 2), dtype=torch.float32, device="cuda") for p in range(P)]
    outs = [dict(recs=torch.zeros((rows, 4), **i32), cnt=torch.zeros(P, **i32)) for _ in range(2)]
    vpairs = [(dxy[0].data_ptr(), nqs[p], dxy[p + 1].data_ptr(), nts[p]) for p in range(P)]
    pos = [(dxy[0].data_ptr(), dxy[p + 1].data_ptr()) for p in range(P)]
    ppos = [(proj[p].data_ptr(), dxy[p + 1].data_ptr()) for p in range(P)]

    def head(model):
        m.match_list_batched(qp, nqs, tp, nts, lst.data_ptr(), cnt.data_ptr(), st)
        fn = v.verify_homography_batched_device if model == "h" else v.verify_batched_device
        fn(lst.data_ptr(), cnt.data_ptr(), vpairs, res.data_ptr(), 0, 0, 0, 1.5, K, 0, 2, 2, st)

    def h_batched():
        head("h")
        sift.project_homography_batched_device(res.data_ptr(), [(dxy[0].data_ptr(), nqs[p], proj[p].data_ptr())
                                                                for p in range(P)], 2, 2, 52, st)
        m.match_list_guided_batched(qp, nqs, tp, nts, ppos, RADIUS, outs[0]["recs"].data_ptr(), outs[0]["cnt"].data_ptr(), 2,
                                    2, st)

    def h_loop():
        head("h")
        for p in range(P):
            sift.project_homography_device(res.data_ptr() + 52 * p, dxy[0].data_ptr(), nqs[p], proj[p].data_ptr(), 2, 2, st)
            m.match_list_guided_device(qp[p], nqs[p], tp[p], nts[p], ppos[p][0], ppos[p][1], RADIUS,
                                       outs[1]["recs"].data_ptr() + 16 * int(row0[p]), outs[1]["cnt"].data_ptr() + 4 * p, 2, 2,
                                       st)

    def f_batched():
        head("f")
        m.match_list_epipolar_batched(qp, nqs, tp, nts, pos, res.data_ptr(), max_error, outs[0]["recs"].data_ptr(),
                                      outs[0]["cnt"].data_ptr(), INF, 52, 2, 2, st)

    def f_loop():
        head("f")
        rec = res.cpu().numpy().view(sift.VERIFY_RESULT_DTYPE).reshape(-1)  # the read-back: a host synchronisation
        for p in range(P):
            if not cv.geometry_usable(rec[p]["F"]):
                outs[1]["cnt"][p] = 0
                continue
            m.match_list_epipolar_device(qp[p], nqs[p], tp[p], nts[p], pos[p][0], pos[p][1], rec[p]["F"], max_error,
                                         outs[1]["recs"].data_ptr() + 16 * int(row0[p]), outs[1]["cnt"].data_ptr() + 4 * p,
                                         INF, 2, 2, st)

    out = {"pairs": P, "hypotheses": K, "rows_per_set": ns}
    for name, fb, fl in (("h", h_batched, h_loop), ("f", f_batched, f_loop)):
        for o in outs:
            for t in o.values():
                t.zero_()
        fb(), fl()
        torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in outs)
        if a["cnt"].tobytes() != b["cnt"].tobytes():
            raise SystemExit(f"chain {name}: the batched counts differ from the loop's: nothing to time")
        ra, rb = (x["recs"].copy().view(sift.DMATCH_DTYPE).reshape(-1) for x in (a, b))
        for p in range(P):
            x, y = (r[row0[p]:row0[p] + int(a["cnt"][p])].copy() for r in (ra, rb))
            x["imgIdx"] = 0
            if x.tobytes() != y.tobytes():
                raise SystemExit(f"chain {name} pair {p}: the batched list differs from the loop's: nothing to time")
        t = timed(torch, [(f"{name}_batched", fb, max(calls // 2, 4)), (f"{name}_loop", fl, max(calls // 5, 4))], passes)
        bb, lo = t[f"{name}_batched"], t[f"{name}_loop"]
        out[name] = {"kept": a["cnt"].tolist(), "stream_us": t, "loop_over_batched": round(lo["median"] / bb["median"], 2),
                     "batched_wholly_below_loop": bool(bb["max"] < lo["min"])}
        print(f"chain {name}: {out[name]['loop_over_batched']}", file=sys.stderr, flush=True)
    return out


def child(calls):
    """The single-pair calls alone on foreign buffers (this process's library)."""
    import torch

    world = setup()
    sets, ns, xy, dxy = world
    F = eb.fundamental()
    m = sift.Matcher(N, N, device=0)
    st = torch.cuda.current_stream().cuda_stream
    idx2 = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    d2 = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    a = (sets[0].data_ptr(), ns[0], sets[1].data_ptr(), ns[1])
    xyp = (dxy[0].data_ptr(), dxy[1].data_ptr())
    o = (0.8, False, idx2.data_ptr(), d2.data_ptr(), 0, st)
    legs = [("match_device", lambda: m.match_device(*a, *o)),
            ("match_guided_device", lambda: m.match_guided_device(*a, *xyp, RADIUS, 2, 2, *o)),
            ("match_epipolar_device", lambda: m.match_epipolar_device(*a, *xyp, F, 4.0, INF, 2, 2, *o))]
    for _ in range(20):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _ in legs}
    for _ in range(5):
        for k, fn in legs:
            t[k].append(stream_us(torch, fn, calls))
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
                               capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode or not line:
                raise SystemExit(f"single-pair child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
    out = {"pairs": rows}
    for leg in [k for k in rows[0]["this"] if k != "library"]:
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": eb.summary(a), "parent_us": eb.summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_batched", "match_guided_batched_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("match_guided_batched_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    import torch

    from sift_amd import cv

    world = setup()
    xy = world[2]
    window = float(cv.gate_mask(xy[0], xy[1], RADIUS).sum(1).mean())
    max_error = eb.band_for(xy, eb.fundamental(), window)
    res = {"workload": f"pairs of the descriptor sets of 8 {W}x{H} synthetic frames (77..84, up to {N} rows, foreign fp16 "
                       f"buffers); positions uniform in {W} x {H}; window radius {RADIUS:g} ({window:.2f} candidates per "
                       f"query), max_error {max_error:.4g}; stream_us: back-to-back repetitions between HIP events, per "
                       f"repetition (b*: one batched call, l*: P single-pair calls)",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls, "max_error": max_error,
           "launch_shape": "8 waves x 1 query block per workgroup (the single-pair gated kernels' shape); the 8 x 2 shape "
                           "spills under the two-workgroups-per-CU launch bound and is not built",
           "not_measured": ["the occupancy of the new kernels", "anything beyond one GPU"]}
    res["batched_vs_loop"] = measure(torch, world, max_error, a.passes, a.calls)
    res["chains"] = chains(torch, world, max_error, a.passes, a.calls)
    if a.parent_lib:
        res["single_pair_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, max(a.calls, 200))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
