"""Cost of homography verification (Verifier.verify_homography_device: a fixed-budget 4-point RANSAC on the device)
at 2000 matches x K hypotheses, K in {256, 1024, 4096}, against the fundamental verifier on a list of the same size,
and of the read-back-free chain it closes.

    python3 tools/verify_homography_bench.py [--passes 5] [--calls 200] [--parent-lib PATH]
                                             [--out profiles/homography/verify_homography_bench.json]

The homography list: 1200 pairs of a plane (n = (0.15, -0.1, 1) / |n|, d = 5) seen by tools/verify_bench.py's two
cameras (1920 x 1200, focal length 1400; positions rounded to the quarter pixel) and 800 pairs of unrelated uniform
positions, shuffled, indexing shuffled position arrays.  The fundamental list is tools/verify_bench.py's own (the same
sizes).  Legs, per K, each timed as `calls` back-to-back calls on one stream between two HIP events, per call; passes of
every leg alternate (h256, f256, hs256, fs256, h1024, ...), so clock and neighbour drift hit all alike; reported per
leg: the median of the passes and their range.
    h   verify_homography_device   gather + K hypotheses + K x n score + select, mask and inlier list written
    f   verify_device              the same for the fundamental matrix
    hs  score_homography_device    gather + score alone on the K hypotheses h solved      fs  score_device likewise
Every result is checked first: record, mask, list, hypotheses and counts must equal sift_amd.cv.ransac_homography /
ransac_fundamental byte for byte, the projection cv.project_homography.

The chain, on 2000 x 2000 descriptors of two synthetic frames with uniform positions (the geometry is meaningless, the
work is the same), wall-clock per iteration, each iteration ending synchronised:
    chain_device   match_list_device -> verify_homography_device (count read from the list's device counter) ->
                   project_homography_device (H read from the result record on the device) ->
                   match_list_guided_device on the projected positions: one stream, no read-back
    chain_host     the same through the host: the list's count read back, verify_homography_host (synchronous), the
                   query positions projected by cv.project_homography and uploaded, match_list_guided_device

--parent-lib: a libsift_hip.so built from the parent commit.  verify_device and score_device (fundamental) are then
timed in child processes alternating between this build and that one (SIFT_HIP_LIB), one interleaved pair per pass:
the score and select kernels are now instances of a template shared with the homography, and the ranges should
overlap."""
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
import verify_bench as vb  # noqa: E402  (the fundamental scene, summary())

W, H, N, N_IN, KS, MAX_ERROR = vb.W, vb.H, vb.N, vb.N_IN, vb.KS, vb.MAX_ERROR
RADIUS = 4.0


def plane_scene():
    """(matches, q_xy, t_xy, planted): N records over (N, 2) float32 position arrays, N_IN of them pairs of a plane."""
    rng = np.random.default_rng(12)
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    rvec, t = np.array([0.02, -0.03, 0.01]), np.array([0.6, 0.1, 0.15])
    th = np.linalg.norm(rvec)
    k = rvec / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * (kx @ kx)
    nrm = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
    Ht = K @ (R + np.outer(t, nrm) / 5.0) @ np.linalg.inv(K)
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < N_IN:
        uv = np.rint(rng.uniform(0, (W, H), (4 * N_IN, 2)) * 4) / 4
        p = np.c_[uv, np.ones(len(uv))] @ Ht.T
        s = p[:, :2] / p[:, 2:]
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
    """Both models on lists of the same size, one verifier each (a verifier holds one model's hypotheses at a time)."""

    def __init__(self):
        import torch

        self.torch = torch
        self.st = torch.cuda.current_stream().cuda_stream
        self.host, self.dev = {}, {}
        for model, (m, q_xy, t_xy, planted) in (("h", plane_scene()), ("f", vb.scene())):
            self.host[model] = (m, q_xy, t_xy, planted)
            self.dev[model] = (torch.from_numpy(m.view(np.int32).reshape(N, 4).copy()).cuda(),
                               torch.from_numpy(q_xy).cuda(), torch.from_numpy(t_xy).cuda())
        self.v = {model: sift.Verifier(N, max(KS), device=0) for model in "hf"}
        self.res = torch.zeros(13, dtype=torch.int32, device="cuda")
        self.out = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(max(KS), dtype=torch.int32, device="cuda")
        self.proj = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
        self.Ms = {}

    def verify(self, model, K):
        dm, dq, dt = self.dev[model]
        fn = self.v[model].verify_homography_device if model == "h" else self.v[model].verify_device
        fn(dm.data_ptr(), 0, N, dq.data_ptr(), N, dt.data_ptr(), N, self.res.data_ptr(), self.out.data_ptr(),
           self.cnt.data_ptr(), self.mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, self.st)

    def score(self, model, K):
        dm, dq, dt = self.dev[model]
        fn = self.v[model].score_homography_device if model == "h" else self.v[model].score_device
        fn(dm.data_ptr(), 0, N, dq.data_ptr(), N, dt.data_ptr(), N, self.Ms[model, K].data_ptr(), K, MAX_ERROR,
           self.counts.data_ptr(), 2, 2, self.st)

    def check(self, model, K):
        """The device's result against the numpy rule; keeps the solved hypotheses for the score leg."""
        from sift_amd import cv

        m, q_xy, t_xy, planted = self.host[model]
        self.verify(model, K)
        if model == "h":
            samples, M, valid, counts = self.v[model].homography_hypotheses()
            ref = cv.ransac_homography(m, q_xy, t_xy, MAX_ERROR, K, 0)
            rec, key, keys = self.res.cpu().numpy().view(sift.HOMOGRAPHY_RESULT_DTYPE)[0], "H", "Hs"
        else:
            samples, M, valid, counts = self.v[model].hypotheses()
            ref = cv.ransac_fundamental(m, q_xy, t_xy, MAX_ERROR, K, 0)
            rec, key, keys = self.res.cpu().numpy().view(sift.VERIFY_RESULT_DTYPE)[0], "F", "Fs"
        n = int(self.cnt.cpu()[0])
        if (rec[key].tobytes() != ref[key].tobytes() or rec["hypothesis"] != ref["hypothesis"] or n != ref["inliers"]
                or rec["valid_hypotheses"] != ref["valid_hypotheses"] or not np.array_equal(samples, ref["samples"])
                or M.tobytes() != ref[keys].tobytes() or not np.array_equal(counts, ref["counts"])
                or not np.array_equal(self.mask.cpu().numpy(), ref["mask"])
                or self.out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes() != ref["list"].tobytes()):
            raise SystemExit(f"{model} K = {K}: the device result differs from the reference: nothing to time")
        self.Ms[model, K] = self.torch.from_numpy(M.copy()).cuda()
        self.score(model, K)
        self.torch.cuda.synchronize()
        if not np.array_equal(self.counts.cpu().numpy()[:K], ref["counts"]):
            raise SystemExit(f"{model} K = {K}: the score call differs from the reference: nothing to time")
        if model == "h":
            sift.project_homography_device(self.res.data_ptr(), self.dev["h"][1].data_ptr(), N, self.proj.data_ptr(), 2, 2,
                                           self.st)
            self.torch.cuda.synchronize()
            if self.proj.cpu().numpy().tobytes() != cv.project_homography(ref["H"], q_xy).tobytes():
                raise SystemExit(f"K = {K}: the projection differs from the reference: nothing to time")
        mask = ref["mask"] != 0
        return {"hypothesis": int(ref["hypothesis"]), "inliers": int(ref["inliers"]),
                "valid_hypotheses": int(ref["valid_hypotheses"]),
                "planted_recovered": int((mask & planted).sum()), "outliers_admitted": int((mask & ~planted).sum())}

    def stream_us(self, fn, calls):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        self.torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3


def measure(passes, calls):
    legs = Legs()
    out = {"results": {f"{model}{K}": legs.check(model, K) for K in KS for model in "hf"}}
    names = []
    for K in KS:
        for model in "hf":
            names += [(f"{model}{K}", lambda model=model, K=K: legs.verify(model, K)),
                      (f"{model}s{K}", lambda model=model, K=K: legs.score(model, K))]
    for _ in range(20):
        for _, fn in names:
            fn()
    legs.torch.cuda.synchronize()
    t = {k: [] for k, _ in names}
    for _ in range(passes):
        for k, fn in names:
            t[k].append(legs.stream_us(fn, calls))
    out["stream_us"] = {k: vb.summary(v) for k, v in t.items()}
    out["homography_over_fundamental"] = {}
    for K in KS:
        h, f = out["stream_us"][f"h{K}"], out["stream_us"][f"f{K}"]
        out["homography_over_fundamental"][str(K)] = {
            "ratio_of_medians": round(h["median"] / f["median"], 3),
            "homography_slower_beyond_spread": bool(h["min"] > f["max"])}
    return out


def chain(passes, calls):
    """The four-call chain against the same chain through the host, wall-clock us per iteration."""
    import torch

    from sift_amd import cv

    det = sift.Detector(sift.CudaSiftConfig(col_width=W, row_width=H, numOctaves=3, numFeatures=N), device=0)
    det.gpuWarmUpAndAllocate()
    det.detectAndCompute(sift.synth_frame(77, W, H))
    det.detectAndCompute(sift.synth_frame(78, W, H))
    if min(det.prev_size, det.total_size) < N:
        raise SystemExit(f"the frames gave {det.prev_size} / {det.total_size} keypoints: not the {N} x {N} workload")
    q, t = det.prev_descriptor.data(), det.device_descriptor.data()
    rng = np.random.default_rng(7)
    hxy = [(rng.random((N, 2)) * (W, H)).astype(np.float32) for _ in range(2)]
    dxy = [torch.from_numpy(a).cuda() for a in hxy]
    qxy, txy = dxy[0].data_ptr(), dxy[1].data_ptr()
    m, v, K = sift.Matcher(N, N, max_pairs=1, device=0), sift.Verifier(N, 1024, device=0), 1024
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    lst, cnt, res = torch.zeros((N, 4), **i32), torch.zeros(1, **i32), torch.zeros(13, **i32)
    out, ocnt = torch.zeros((N, 4), **i32), torch.zeros(1, **i32)
    proj = torch.zeros((N, 2), dtype=torch.float32, device="cuda")

    def device():
        m.match_list_device(q, N, t, N, lst.data_ptr(), cnt.data_ptr(), st)
        v.verify_homography_device(lst.data_ptr(), cnt.data_ptr(), N, qxy, N, txy, N, res.data_ptr(), 0, 0, 0, MAX_ERROR, K,
                                   0, 2, 2, st)
        sift.project_homography_device(res.data_ptr(), qxy, N, proj.data_ptr(), 2, 2, st)
        m.match_list_guided_device(q, N, t, N, proj.data_ptr(), txy, RADIUS, out.data_ptr(), ocnt.data_ptr(), 2, 2, st)
        torch.cuda.synchronize()

    def host():
        m.match_list_device(q, N, t, N, lst.data_ptr(), cnt.data_ptr(), st)
        n = int(cnt.cpu()[0])
        Hm, _inl, _hyp = v.verify_homography_host(lst.data_ptr(), 0, n, qxy, N, txy, N, MAX_ERROR, K, 0, 2, 2)
        proj.copy_(torch.from_numpy(cv.project_homography(Hm, hxy[0])))
        m.match_list_guided_device(q, N, t, N, proj.data_ptr(), txy, RADIUS, out.data_ptr(), ocnt.data_ptr(), 2, 2, st)
        torch.cuda.synchronize()

    device()
    rec = res.cpu().numpy().view(sift.HOMOGRAPHY_RESULT_DTYPE)[0]
    a = (out.cpu().numpy().tobytes(), int(ocnt.cpu()[0]), int(cnt.cpu()[0]), proj.cpu().numpy().tobytes())
    host()
    if a != (out.cpu().numpy().tobytes(), int(ocnt.cpu()[0]), int(cnt.cpu()[0]), proj.cpu().numpy().tobytes()):
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
    res_ = {"putative_matches": a[2], "verified_hypothesis": int(rec["hypothesis"]), "verified_inliers": int(rec["inliers"]),
            "guided_matches": a[1], "hypotheses": K, "radius": RADIUS,
            "wall_us_per_iteration": {k: vb.summary(x) for k, x in t_us.items()}}
    res_["host_over_device"] = round(res_["wall_us_per_iteration"]["chain_host"]["median"]
                                     / res_["wall_us_per_iteration"]["chain_device"]["median"], 3)
    return res_


def child(calls):
    """verify_device and score_device (fundamental) alone, on this process's library."""
    import torch

    from sift_amd import cv

    m, q_xy, t_xy, _ = vb.scene()
    dm = torch.from_numpy(m.view(np.int32).reshape(N, 4).copy()).cuda()
    dq, dt = torch.from_numpy(q_xy).cuda(), torch.from_numpy(t_xy).cuda()
    v = sift.Verifier(N, max(KS), device=0)
    st = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device="cuda")
    res, out, cnt = torch.zeros(13, **i32), torch.zeros((N, 4), **i32), torch.zeros(1, **i32)
    mask, counts = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(max(KS), **i32)
    Fs = {}

    def verify(K):
        v.verify_device(dm.data_ptr(), 0, N, dq.data_ptr(), N, dt.data_ptr(), N, res.data_ptr(), out.data_ptr(),
                        cnt.data_ptr(), mask.data_ptr(), MAX_ERROR, K, 0, 2, 2, st)

    def score(K):
        v.score_device(dm.data_ptr(), 0, N, dq.data_ptr(), N, dt.data_ptr(), N, Fs[K].data_ptr(), K, MAX_ERROR,
                       counts.data_ptr(), 2, 2, st)

    def stream_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls * 1e3

    result = {"library": sift.version()}
    for K in KS:
        verify(K)
        _, F, _, c = v.hypotheses()
        ref = cv.ransac_fundamental(m, q_xy, t_xy, MAX_ERROR, K, 0)
        if F.tobytes() != ref["Fs"].tobytes() or not np.array_equal(c, ref["counts"]) or \
                not np.array_equal(mask.cpu().numpy(), ref["mask"]):
            raise SystemExit(f"child K = {K}: the device result differs from the reference")
        Fs[K] = torch.from_numpy(F.copy()).cuda()
    for _ in range(20):
        for K in KS:
            verify(K)
            score(K)
    torch.cuda.synchronize()
    for K in KS:
        result[f"verify_device_{K}"] = round(float(np.median([stream_us(lambda: verify(K)) for _ in range(3)])), 2)
        result[f"score_device_{K}"] = round(float(np.median([stream_us(lambda: score(K)) for _ in range(3)])), 2)
    print("CHILD " + json.dumps(result), flush=True)


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
                raise SystemExit(f"fundamental-path child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
            pair[name] = json.loads(line[-1][6:])
        rows.append(pair)
        print(f"pair {len(rows)} of {passes} done", file=sys.stderr, flush=True)
    out = {"pairs": rows}
    for leg in [f"{k}_{K}" for K in KS for k in ("verify_device", "score_device")]:
        a, b = [p["this"][leg] for p in rows], [p["parent"][leg] for p in rows]
        out[leg] = {"this_us": vb.summary(a), "parent_us": vb.summary(b),
                    "this_over_parent": round(float(np.median(a)) / float(np.median(b)), 3),
                    "ranges_overlap": bool(min(a) <= max(b) and min(b) <= max(a))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography", "verify_homography_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_homography_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    res = {"workload": f"{N} matches ({N_IN} pairs of a plane seen by two synthetic cameras + {N - N_IN} pairs of "
                       f"unrelated positions, {W} x {H}; the fundamental legs: tools/verify_bench.py's list of the same "
                       f"sizes), max_error {MAX_ERROR}, seed 0; stream_us: {a.calls} back-to-back calls between HIP "
                       f"events, per call",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls}
    res.update(measure(a.passes, a.calls))
    print("legs done", file=sys.stderr, flush=True)
    res["chain"] = chain(a.passes, a.calls)
    print("chain done", file=sys.stderr, flush=True)
    if a.parent_lib:
        res["fundamental_path_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
