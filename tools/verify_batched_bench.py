"""Cost of batched two-view verification (Verifier.verify_batched_device / verify_homography_batched_device: all P
pairs of a match batch in one gather, one hypotheses, one score and one select launch) against the same P pairs through
P single-pair calls, at the shapes of the all-pairs exchange: P = 7 (one GPU's share of 8 sets) and P = 56 (all ordered
pairs), 2000 matches per pair, K in {256, 1024, 4096}, both models.

    python3 tools/verify_batched_bench.py [--passes 5] [--calls 100] [--parent-lib PATH]
                                          [--out profiles/verify_batched/verify_batched_bench.json]
    python3 tools/verify_batched_bench.py --trace f|h P K [--calls 100]   (under a kernel trace: only batched calls, for
                                                                           the per-kernel split)

Each pair's list is the existing tools' scene -- tools/verify_bench.py's 1200 true pairs of a two-camera scene and 800
pairs of unrelated positions (tools/verify_homography_bench.py's plane for the homography) -- in an order of its own
(a permutation seeded by p), over its own copy of the position arrays.  Legs, per model, P and K:
    b   one batched call                       4 launches for all P pairs, pair p with the seed p
    l   P single-pair calls, back to back      4 P launches on the same stream and the same verifier, seeds 0 .. P - 1;
                                               the single-pair path is the parent commit's code, unchanged
Before anything is timed every pair's result record, out rows, out count and mask of b must equal l's byte for byte (and,
at P = 7 and K = 256, the numpy rule sift_amd.cv.ransac_* with the seed p).  Each leg is timed as `calls` (l: calls / 5)
back-to-back repetitions on one stream between two HIP events; passes of the legs alternate (b, l, b, l, ...), so clock
and neighbour drift hit both alike; reported per leg: the median of the passes and their range, loop over batched as
the ratio of the medians, and whether the batched call's range lies wholly below the loop's.

The chain, on the descriptors of 8 synthetic frames (1920 x 1200, up to 2000 rows each) with uniform positions (the
geometry is meaningless, the work is the same), P = 7, K = 1024, the homography: match_list_batched ->
verify_homography_batched_device with cap[p] = nq[p] and the list's device counters, on one stream with no read-back,
timed as the two calls together, each alone, and against match_list_batched followed by 7 single verify calls.

--parent-lib: a libsift_hip.so built from the parent commit (tools/ab_build.sh).  The single-pair calls verify_device
and score_device at K = 256 / 1024 / 4096 and verify_homography_device are then timed in child processes alternating
between this build and that one (SIFT_HIP_LIB), one interleaved pair per pass: their kernels are now the single-list
instantiations of templates shared with the batched ones, and the ranges should overlap."""
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
import verify_bench as vb  # noqa: E402  (the fundamental scene, summary())
import verify_homography_bench as vhb  # noqa: E402  (the plane scene)

W, H, N, KS, MAX_ERROR = vb.W, vb.H, vb.N, vb.KS, vb.MAX_ERROR
PS = (7, 56)


def stream_us(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


class Batch:
    """P lists of one model on the device, a batched verifier, and two sets of outputs (the batched call's, the
    loop's)."""

    def __init__(self, model, P):
        import torch

        self.torch, self.model, self.P = torch, model, P
        self.st = torch.cuda.current_stream().cuda_stream
        m, q_xy, t_xy, _ = vhb.plane_scene() if model == "h" else vb.scene()
        self.lists = [m[np.random.default_rng(100 + p).permutation(N)] for p in range(P)]
        self.q_xy, self.t_xy = q_xy, t_xy
        rows = np.concatenate(self.lists).view(np.int32).reshape(P * N, 4)
        self.dm = torch.from_numpy(rows.copy()).cuda()
        self.dq = [torch.from_numpy(q_xy).cuda() for _ in range(P)]
        self.dt = [torch.from_numpy(t_xy).cuda() for _ in range(P)]
        self.pairs = [(self.dq[p].data_ptr(), N, self.dt[p].data_ptr(), N, N) for p in range(P)]
        self.v = sift.Verifier(P * N, max(KS), P, device=0)
        i32 = dict(dtype=torch.int32, device="cuda")
        self.outs = [dict(res=torch.zeros((P, 13), **i32), out=torch.zeros((P * N, 4), **i32), cnt=torch.zeros(P, **i32),
                          mask=torch.zeros(P * N, dtype=torch.uint8, device="cuda")) for _ in range(2)]

    def zero(self):
        for o in self.outs:
            for t in o.values():
                t.zero_()

    def batched(self, K):
        o = self.outs[0]
        fn = self.v.verify_homography_batched_device if self.model == "h" else self.v.verify_batched_device
        fn(self.dm.data_ptr(), 0, self.pairs, o["res"].data_ptr(), o["out"].data_ptr(), o["cnt"].data_ptr(),
           o["mask"].data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def loop(self, K):
        o = self.outs[1]
        fn = self.v.verify_homography_device if self.model == "h" else self.v.verify_device
        dm, res, out, cnt, mask = (t.data_ptr() for t in (self.dm, o["res"], o["out"], o["cnt"], o["mask"]))
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            fn(dm + 16 * N * p, 0, cap, q, nq, t, nt, res + 52 * p, out + 16 * N * p, cnt + 4 * p, mask + N * p, MAX_ERROR,
               K, p, 2, 2, self.st)

    def check(self, K):
        """The batched call's bytes against the loop's, every pair; at P = 7 and the smallest K also against the rule."""
        from sift_amd import cv

        self.zero()
        self.batched(K)
        self.loop(K)
        self.torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in self.outs)
        for k in a:
            if a[k].tobytes() != b[k].tobytes():
                raise SystemExit(f"{self.model} P = {self.P} K = {K}: the batched call's {k} differs from the loop's: "
                                 "nothing to time")
        dtype = sift.HOMOGRAPHY_RESULT_DTYPE if self.model == "h" else sift.VERIFY_RESULT_DTYPE
        rec = a["res"].view(dtype).reshape(-1)
        if self.P == min(PS) and K == min(KS):
            rule, key = (cv.ransac_homography, "H") if self.model == "h" else (cv.ransac_fundamental, "F")
            recs = a["out"].view(sift.DMATCH_DTYPE).reshape(-1)
            for p in range(self.P):
                ref = rule(self.lists[p], self.q_xy, self.t_xy, MAX_ERROR, K, p)
                n = int(a["cnt"][p])
                if (rec[p][key].tobytes() != ref[key].tobytes() or rec[p]["hypothesis"] != ref["hypothesis"]
                        or n != ref["inliers"] or recs[N * p: N * p + n].tobytes() != ref["list"].tobytes()
                        or not np.array_equal(a["mask"][N * p: N * (p + 1)], ref["mask"])):
                    raise SystemExit(f"{self.model} pair {p}: the device result differs from the rule: nothing to time")
        return {"winners": int((rec["hypothesis"] >= 0).sum()), "inliers_min": int(rec["inliers"].min()),
                "inliers_max": int(rec["inliers"].max()), "distinct_hypotheses": len(set(rec["hypothesis"].tolist()))}


def measure(passes, calls):
    import torch

    out = {}
    for model in "fh":
        for P in PS:
            b = Batch(model, P)
            checks = {str(K): b.check(K) for K in KS}
            names = []
            for K in KS:
                names += [(f"b{K}", lambda K=K: b.batched(K), calls), (f"l{K}", lambda K=K: b.loop(K), max(calls // 5, 4))]
            for _ in range(5):
                for _, fn, _c in names:
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k, _, _ in names}
            for _ in range(passes):
                for k, fn, c in names:
                    t[k].append(stream_us(torch, fn, c))
            leg = {"checked": checks, "stream_us": {k: vb.summary(v) for k, v in t.items()}, "loop_over_batched": {}}
            for K in KS:
                bb, ll = leg["stream_us"][f"b{K}"], leg["stream_us"][f"l{K}"]
                leg["loop_over_batched"][str(K)] = {
                    "ratio_of_medians": round(ll["median"] / bb["median"], 2),
                    "loop_us_per_pair": round(ll["median"] / P, 2), "batched_us_per_pair": round(bb["median"] / P, 2),
                    "batched_wholly_below_loop": bool(bb["max"] < ll["min"])}
            out[f"{model}_P{P}"] = leg
            print(f"measured {model} P = {P}: {leg['loop_over_batched']}", file=sys.stderr, flush=True)
            del b
    return out


def chain(passes, calls):
    """match_list_batched -> verify_homography_batched_device on one stream, P = 7: one GPU's share of 8 sets."""
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
    dxy = [torch.from_numpy((rng.random((N, 2)) * (W, H)).astype(np.float32)).cuda() for _ in range(8)]
    P, K = 7, 1024
    qp, nqs = [sets[0].data_ptr()] * P, [ns[0]] * P
    tp, nts = [sets[j].data_ptr() for j in range(1, 8)], ns[1:]
    rows = sum(nqs)
    m, v = sift.Matcher(N, N, max_pairs=P, device=0), sift.Verifier(rows, K, P, device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    lst, cnt = torch.zeros((rows, 4), **i32), torch.zeros(P, **i32)
    outs = [dict(res=torch.zeros((P, 13), **i32), out=torch.zeros((rows, 4), **i32), cnt=torch.zeros(P, **i32))
            for _ in range(2)]
    pairs = [(dxy[0].data_ptr(), nqs[p], dxy[p + 1].data_ptr(), nts[p]) for p in range(P)]
    row0 = np.concatenate([[0], np.cumsum(nqs)]).astype(int)

    def match():
        m.match_list_batched(qp, nqs, tp, nts, lst.data_ptr(), cnt.data_ptr(), st)

    def verify():
        o = outs[0]
        v.verify_homography_batched_device(lst.data_ptr(), cnt.data_ptr(), pairs, o["res"].data_ptr(), o["out"].data_ptr(),
                                           o["cnt"].data_ptr(), 0, MAX_ERROR, K, 0, 2, 2, st)

    def verify_loop():
        o = outs[1]
        for p, (q, nq, t, nt) in enumerate(pairs):
            v.verify_homography_device(lst.data_ptr() + 16 * int(row0[p]), cnt.data_ptr() + 4 * p, nq, q, nq, t, nt,
                                       o["res"].data_ptr() + 52 * p, o["out"].data_ptr() + 16 * int(row0[p]),
                                       o["cnt"].data_ptr() + 4 * p, 0, MAX_ERROR, K, p, 2, 2, st)

    def both():
        match()
        verify()

    def both_loop():
        match()
        verify_loop()

    both()
    verify_loop()
    torch.cuda.synchronize()
    for k in outs[0]:
        if outs[0][k].cpu().numpy().tobytes() != outs[1][k].cpu().numpy().tobytes():
            raise SystemExit(f"chain: the batched call's {k} differs from the loop's: nothing to time")
    legs = [("match_list_batched", match, calls), ("verify_batched", verify, calls), ("chain_batched", both, calls),
            ("chain_loop", both_loop, max(calls // 5, 4))]
    for _ in range(5):
        for _, fn, _c in legs:
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in legs}
    for _ in range(passes):
        for k, fn, c in legs:
            t[k].append(stream_us(torch, fn, c))
    res = {"pairs": P, "hypotheses": K, "rows_per_set": ns, "putative_matches": cnt.cpu().numpy().tolist(),
           "inliers": outs[0]["cnt"].cpu().numpy().tolist(), "stream_us": {k: vb.summary(x) for k, x in t.items()}}
    res["chain_loop_over_chain_batched"] = round(res["stream_us"]["chain_loop"]["median"]
                                                 / res["stream_us"]["chain_batched"]["median"], 2)
    return res


def child(calls):
    """The single-pair calls alone (this process's library): verify_device and score_device at every K,
    verify_homography_device at every K."""
    import torch

    f, h = vb.Legs(), vhb.Legs()
    legs = []
    for K in KS:
        f.check(K)
        h.check("h", K)
        legs += [(f"verify_device_{K}", lambda K=K: f.verify(K)), (f"score_device_{K}", lambda K=K: f.score(K)),
                 (f"verify_homography_device_{K}", lambda K=K: h.verify("h", K))]
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


def trace(model, P, K, calls):
    b = Batch(model, P)
    b.check(K)
    for _ in range(calls):
        b.batched(K)
    b.torch.cuda.synchronize()
    print(f"TRACE model={model} P={P} K={K} batched calls={calls + 1}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", nargs=3, metavar=("MODEL", "P", "K"))
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batched", "verify_batched_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_batched_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    if a.trace:
        trace(a.trace[0], int(a.trace[1]), int(a.trace[2]), a.calls)
        return
    res = {"workload": f"P pairs of {N} matches each (the scenes of tools/verify_bench.py and "
                       f"tools/verify_homography_bench.py, a record order per pair), max_error {MAX_ERROR}, seed 0 (pair p: "
                       f"seed p); stream_us: back-to-back repetitions between HIP events, per repetition (b: one batched "
                       f"call, l: P single-pair calls)",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls}
    res["batched_vs_loop"] = measure(a.passes, a.calls)
    if not a.no_chain:
        res["chain"] = chain(a.passes, a.calls)
    if a.parent_lib:
        res["single_pair_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, max(a.calls, 200))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
