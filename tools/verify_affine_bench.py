"""Cost of affine and similarity verification (Verifier.verify_affine_device: a fixed-budget 3- / 2-point RANSAC on the
device), of its score and of its refit, against the homography calls of the same build in the same passes.

    python3 tools/verify_affine_bench.py [--passes 5] [--calls 200] [--parent-lib PATH]
                                         [--out profiles/affine/verify_affine_bench.json]

The lists have the shape of tools/verify_homography_bench.py's: 2000 records over shuffled position arrays, 1200 pairs
planted under a true map in 1920 x 1200 (positions rounded to the quarter pixel) and 800 pairs of unrelated uniform
positions.  The affine legs' map is R(17 deg) [[1.2, 0.18], [0, 0.85]] about the frame's centre plus (6, -4), the
similarity legs' 1.15 R(17 deg) about the centre plus (6, -4); the homography legs run on
tools/verify_homography_bench.py's plane.  Every result is checked first: record, mask, list, hypotheses and counts
must equal sift_amd.cv.ransac_affine (ransac_homography) byte for byte, the refit cv.refine_affine
(refine_homography).  Each leg is timed as `calls` back-to-back calls on one stream between two HIP events, per call;
the passes of a group's legs alternate, so clock and neighbour drift hit all alike; reported per leg: the median of the
passes and their range.

single    per K in {256, 1024, 4096}: verify_affine_device for the affine map (a) and the similarity (s),
          verify_homography_device (h); the scores alone on the hypotheses those calls solved: score_affine_device (as),
          score_homography_device (hs).
refit     K = 1024: the verify call alone (v_*), the verify call followed by one refit round (vr_*: the refit starts from
          the verify call's state every time; a round costs vr - v), and the round alone on the state it left (r_*), for
          refine_affine_device (a, s) and refine_homography_device (h).
batched   P = 7 and P = 56, K = 1024: one verify_affine_batched_device call against P single calls on the same stream
          and verifier, both models; one refine_affine_batched_device call against P single refine calls.
--parent-lib  a libsift_hip.so built from the parent commit (tools/ab_build.sh): verify_device, verify_homography_device
          and refine_homography_device in child processes alternating between this build and that one (SIFT_HIP_LIB), one
          interleaved pair per pass; their kernels' bodies did not change and the ranges should overlap.
Not measured: occupancy or any other counter, a kernel trace, the chain with the matcher, anything beyond one GPU, the
C++ surface."""
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
import verify_bench as vb  # noqa: E402  (the fundamental scene, summary())
import verify_homography_bench as vhb  # noqa: E402  (the plane scene)
from sift_amd import cv  # noqa: E402

W, H, N, N_IN, KS, MAX_ERROR = vb.W, vb.H, vb.N, vb.N_IN, vb.KS, vb.MAX_ERROR
K_REFIT, PS = 1024, (7, 56)
MODELS = ("a", "s", "h")  # affine map, similarity, homography


def affine_scene(similarity):
    """(matches, q_xy, t_xy, planted): N records over (N, 2) float32 position arrays, N_IN of them pairs of the map."""
    rng = np.random.default_rng(21 + similarity)
    c, s = np.cos(np.deg2rad(17.0)), np.sin(np.deg2rad(17.0))
    R = np.array([[c, -s], [s, c]])
    A = 1.15 * R if similarity else R @ np.array([[1.2, 0.18], [0.0, 0.85]])
    centre = np.array([W / 2.0, H / 2.0])
    shift = centre - A @ centre + np.array([6.0, -4.0])
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < N_IN:
        uv = np.rint(rng.uniform(0, (W, H), (4 * N_IN, 2)) * 4) / 4
        im = uv @ A.T + shift
        ok = ((im >= 0) & (im < (W, H))).all(1)
        a, b = np.r_[a, uv[ok]], np.r_[b, im[ok]]
    q_xy = rng.uniform(0, (W, H), (N, 2))
    t_xy = rng.uniform(0, (W, H), (N, 2))
    qrow, trow = rng.permutation(N), rng.permutation(N)
    q_xy[qrow[:N_IN]], t_xy[trow[:N_IN]] = a[:N_IN], b[:N_IN]
    order = rng.permutation(N)
    m = np.zeros(N, sift.DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["distance"] = qrow[order], trow[order], 1.0
    grid = lambda p: (np.rint(p * 4) / 4).astype(np.float32)  # noqa: E731
    return m, grid(q_xy), grid(t_xy), order < N_IN


def scene(model):
    return vhb.plane_scene() if model == "h" else affine_scene(model == "s")


def rules(model):
    """(ransac, refine) of a model, with the homography's signatures."""
    if model == "h":
        return cv.ransac_homography, cv.refine_homography
    sim = model == "s"
    return (lambda m, q, t, e, K, seed: cv.ransac_affine(m, q, t, e, K, seed, sim),
            lambda m, q, t, r, e, rounds: cv.refine_affine(m, q, t, r, e, rounds, sim))


def record(d):
    r = np.zeros(1, sift.HOMOGRAPHY_RESULT_DTYPE)
    r["H"][0] = d["H"]
    for k in ("inliers", "hypothesis", "matches", "valid_hypotheses"):
        r[k][0] = d[k]
    return r


def rms_px(M, pts):
    p = np.c_[pts[:, :2], np.ones(len(pts))] @ np.asarray(M, np.float64).reshape(3, 3).T
    return round(float(np.sqrt((((p[:, :2] / p[:, 2:]) - pts[:, 2:]) ** 2).sum(1).mean())), 4)


class Calls:
    """A verifier's verify, score and refine calls for one of the three models (the affine two differ in one keyword)."""

    def __init__(self, v, model):
        kw = {} if model == "h" else {"similarity": model == "s"}
        pick = lambda h, a: (lambda *args: getattr(v, h if model == "h" else a)(*args, **kw))  # noqa: E731
        self.verify = pick("verify_homography_device", "verify_affine_device")
        self.score = pick("score_homography_device", "score_affine_device")
        self.refine = pick("refine_homography_device", "refine_affine_device")
        self.verify_batched = pick("verify_homography_batched_device", "verify_affine_batched_device")
        self.refine_batched = pick("refine_homography_batched_device", "refine_affine_batched_device")
        self.hypotheses = v.homography_hypotheses if model == "h" else (lambda: v.affine_hypotheses(model == "s"))


class Single:
    """One list of a model on the device, its verifier and outputs."""

    def __init__(self, model):
        import torch

        self.torch, self.model = torch, model
        self.m, self.q_xy, self.t_xy, self.planted = scene(model)
        self.dm = torch.from_numpy(self.m.view(np.int32).reshape(N, 4).copy()).cuda()
        self.dq, self.dt = torch.from_numpy(self.q_xy).cuda(), torch.from_numpy(self.t_xy).cuda()
        self.v = sift.Verifier(N, max(KS), device=0)
        self.call = Calls(self.v, model)
        self.st = torch.cuda.current_stream().cuda_stream
        i32 = dict(dtype=torch.int32, device="cuda")
        self.res, self.out, self.ints = torch.zeros(13, **i32), torch.zeros((N, 4), **i32), torch.zeros(2, **i32)
        self.mask = torch.zeros(N, dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(max(KS), **i32)
        self.args = (self.dm.data_ptr(), 0, N, self.dq.data_ptr(), N, self.dt.data_ptr(), N)
        self.Ms = {}

    def verify(self, K):
        self.call.verify(*self.args, self.res.data_ptr(), self.out.data_ptr(), self.ints.data_ptr(), self.mask.data_ptr(),
                         MAX_ERROR, K, 0, 2, 2, self.st)

    def score(self, K):
        self.call.score(*self.args, self.Ms[K].data_ptr(), K, MAX_ERROR, self.counts.data_ptr(), 2, 2, self.st)

    def refine(self, rounds=1):
        self.call.refine(*self.args, self.res.data_ptr(), self.mask.data_ptr(), self.out.data_ptr(), self.ints.data_ptr(),
                         self.ints.data_ptr() + 4, MAX_ERROR, rounds, 2, 2, self.st)

    def listed(self, n):
        return self.out.cpu().numpy().view(sift.DMATCH_DTYPE).reshape(-1)[:n].tobytes()

    def check(self, K):
        """The device's verify and score results against the numpy rule; keeps the hypotheses for the score leg."""
        ransac, _ = rules(self.model)
        self.verify(K)
        samples, M, valid, counts = self.call.hypotheses()
        ref = ransac(self.m, self.q_xy, self.t_xy, MAX_ERROR, K, 0)
        n = int(self.ints.cpu()[0])
        if (self.res.cpu().numpy().tobytes() != record(ref).tobytes() or n != ref["inliers"]
                or not np.array_equal(samples, ref["samples"]) or M.tobytes() != ref["Hs"].tobytes()
                or not np.array_equal(counts, ref["counts"]) or not np.array_equal(self.mask.cpu().numpy(), ref["mask"])
                or self.listed(n) != ref["list"].tobytes()):
            raise SystemExit(f"{self.model} K = {K}: the device result differs from the reference: nothing to time")
        self.Ms[K] = self.torch.from_numpy(M.copy()).cuda()
        self.score(K)
        self.torch.cuda.synchronize()
        if not np.array_equal(self.counts.cpu().numpy()[:K], ref["counts"]):
            raise SystemExit(f"{self.model} K = {K}: the score call differs from the reference: nothing to time")
        mask = ref["mask"] != 0
        return {"hypothesis": int(ref["hypothesis"]), "inliers": int(ref["inliers"]),
                "valid_hypotheses": int(ref["valid_hypotheses"]), "planted_recovered": int((mask & self.planted).sum()),
                "outliers_admitted": int((mask & ~self.planted).sum())}

    def check_refit(self):
        """verify -> one refit round against the rule; the quality numbers."""
        ransac, refine = rules(self.model)
        ref0 = ransac(self.m, self.q_xy, self.t_xy, MAX_ERROR, K_REFIT, 0)
        ref = refine(self.m, self.q_xy, self.t_xy, ref0, MAX_ERROR, 1)
        self.verify(K_REFIT)
        self.refine(1)
        self.torch.cuda.synchronize()
        ints = self.ints.cpu().numpy()
        n = int(ints[0])
        if (self.res.cpu().numpy().tobytes() != record(ref).tobytes() or int(ints[1]) != ref["accepted"]
                or not np.array_equal(self.mask.cpu().numpy(), ref["mask"]) or n != len(ref["list"])
                or self.listed(n) != ref["list"].tobytes()):
            raise SystemExit(f"{self.model}: the device refit differs from the rule: nothing to time")
        pts = cv._match_points(self.m, self.q_xy, self.t_xy).astype(np.float64)[self.planted]
        return {"accepted": int(ref["accepted"]), "inliers_before": int(ref0["inliers"]), "inliers_after": int(ref["inliers"]),
                "planted_rms_px_before": rms_px(ref0["H"], pts), "planted_rms_px_after": rms_px(ref["H"], pts)}


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


def wholly_above(a, b):
    """a's range lies wholly above b's."""
    return bool(a["min"] > b["max"])


def single(passes, calls):
    import torch

    s = {model: Single(model) for model in MODELS}
    out = {"results": {f"{model}{K}": s[model].check(K) for K in KS for model in MODELS}}
    legs = []
    for K in KS:
        legs += [(f"{model}{K}", lambda model=model, K=K: s[model].verify(K), calls) for model in MODELS]
        legs += [(f"{model}s{K}", lambda model=model, K=K: s[model].score(K), calls) for model in ("a", "h")]
    us = out["stream_us"] = timed(torch, legs, passes)
    out["affine_score_against_homography_score"] = {
        str(K): {"ratio_of_medians": round(us[f"as{K}"]["median"] / us[f"hs{K}"]["median"], 3),
                 "affine_wholly_above": wholly_above(us[f"as{K}"], us[f"hs{K}"])} for K in KS}
    out["verify_against_homography"] = {
        str(K): {model: round(us[f"{model}{K}"]["median"] / us[f"h{K}"]["median"], 3) for model in "as"} for K in KS}
    print(f"single: {out['affine_score_against_homography_score']}", file=sys.stderr, flush=True)

    quality = {model: s[model].check_refit() for model in MODELS}

    def vr(model):
        s[model].verify(K_REFIT)
        s[model].refine(1)

    legs = []
    for model in MODELS:
        legs += [(f"v_{model}", lambda model=model: s[model].verify(K_REFIT), calls),
                 (f"vr_{model}", lambda model=model: vr(model), calls),
                 (f"r_{model}", lambda model=model: s[model].refine(1), calls)]
    us = timed(torch, legs, passes)
    refit = {"quality": quality, "stream_us": us,
             "round_cost_us": {model: round(us[f"vr_{model}"]["median"] - us[f"v_{model}"]["median"], 2) for model in MODELS}}
    refit["round_alone_wholly_below_homography"] = {model: bool(us[f"r_{model}"]["max"] < us["r_h"]["min"]) for model in "as"}
    print(f"refit: {refit['round_cost_us']} {refit['round_alone_wholly_below_homography']}", file=sys.stderr, flush=True)
    return out, refit


class Batch:
    """P orders of a model's list on the device, a batched verifier, and two sets of outputs (the batched call's, the
    loop's)."""

    def __init__(self, model, P):
        import torch

        self.torch, self.model, self.P = torch, model, P
        self.st = torch.cuda.current_stream().cuda_stream
        m, self.q_xy, self.t_xy, _ = scene(model)
        self.lists = [m[np.random.default_rng(100 + p).permutation(N)] for p in range(P)]
        self.dm = torch.from_numpy(np.concatenate(self.lists).view(np.int32).reshape(P * N, 4).copy()).cuda()
        self.dq = [torch.from_numpy(self.q_xy).cuda() for _ in range(P)]
        self.dt = [torch.from_numpy(self.t_xy).cuda() for _ in range(P)]
        self.pairs = [(self.dq[p].data_ptr(), N, self.dt[p].data_ptr(), N, N) for p in range(P)]
        self.v = sift.Verifier(P * N, K_REFIT, P, device=0)
        self.call = Calls(self.v, model)
        i32 = dict(dtype=torch.int32, device="cuda")
        self.outs = [dict(res=torch.zeros((P, 13), **i32), out=torch.zeros((P * N, 4), **i32), cnt=torch.zeros(P, **i32),
                          mask=torch.zeros(P * N, dtype=torch.uint8, device="cuda"), acc=torch.zeros(P, **i32))
                     for _ in range(2)]

    def verify_batched(self):
        o = self.outs[0]
        self.call.verify_batched(self.dm.data_ptr(), 0, self.pairs, o["res"].data_ptr(), o["out"].data_ptr(),
                                 o["cnt"].data_ptr(), o["mask"].data_ptr(), MAX_ERROR, K_REFIT, 0, 2, 2, self.st)

    def verify_loop(self):
        o = self.outs[1]
        dm, res, out, cnt, mask = (t.data_ptr() for t in (self.dm, o["res"], o["out"], o["cnt"], o["mask"]))
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            self.call.verify(dm + 16 * N * p, 0, cap, q, nq, t, nt, res + 52 * p, out + 16 * N * p, cnt + 4 * p, mask + N * p,
                             MAX_ERROR, K_REFIT, p, 2, 2, self.st)

    def refine_batched(self):
        o = self.outs[0]
        self.call.refine_batched(self.dm.data_ptr(), 0, self.pairs, o["res"].data_ptr(), o["mask"].data_ptr(),
                                 o["out"].data_ptr(), o["cnt"].data_ptr(), o["acc"].data_ptr(), MAX_ERROR, 1, 2, 2, self.st)

    def refine_loop(self):
        o = self.outs[1]
        dm, res, out, cnt, mask, acc = (t.data_ptr() for t in (self.dm, o["res"], o["out"], o["cnt"], o["mask"], o["acc"]))
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            self.call.refine(dm + 16 * N * p, 0, cap, q, nq, t, nt, res + 52 * p, mask + N * p, out + 16 * N * p, cnt + 4 * p,
                             acc + 4 * p, MAX_ERROR, 1, 2, 2, self.st)

    def same(self, what):
        self.torch.cuda.synchronize()
        a, b = ({k: t.cpu().numpy() for k, t in o.items()} for o in self.outs)
        for k in a:
            if a[k].tobytes() != b[k].tobytes():
                raise SystemExit(f"{self.model} P = {self.P}: the batched {what}'s {k} differs from the loop's: nothing to time")
        return a

    def check(self):
        """The batched calls' bytes against the loops', every pair; at P = 7 also against the rule."""
        ransac, refine = rules(self.model)
        self.verify_batched()
        self.verify_loop()
        a = self.same("verify call")
        refs = []
        if self.P == min(PS):
            rec = a["res"].view(sift.HOMOGRAPHY_RESULT_DTYPE).reshape(-1)
            for p in range(self.P):
                refs.append(ransac(self.lists[p], self.q_xy, self.t_xy, MAX_ERROR, K_REFIT, p))
                if (rec[p:p + 1].tobytes() != record(refs[p]).tobytes()
                        or not np.array_equal(a["mask"][N * p: N * (p + 1)], refs[p]["mask"])):
                    raise SystemExit(f"{self.model} pair {p}: the batched verify call differs from the rule: nothing to time")
        self.refine_batched()
        self.refine_loop()
        a = self.same("refine call")
        rec = a["res"].view(sift.HOMOGRAPHY_RESULT_DTYPE).reshape(-1)
        for p, ref0 in enumerate(refs):
            ref = refine(self.lists[p], self.q_xy, self.t_xy, ref0, MAX_ERROR, 1)
            if (rec[p:p + 1].tobytes() != record(ref).tobytes() or a["acc"][p] != ref["accepted"]
                    or not np.array_equal(a["mask"][N * p: N * (p + 1)], ref["mask"])):
                raise SystemExit(f"{self.model} pair {p}: the batched refit differs from the rule: nothing to time")
        return {"winners": int((rec["hypothesis"] >= 0).sum()), "accepted_pairs": int((a["acc"] > 0).sum()),
                "inliers_min": int(rec["inliers"].min()), "inliers_max": int(rec["inliers"].max())}


def batched(passes, calls):
    import torch

    out = {}
    for model in "as":
        for P in PS:
            b = Batch(model, P)
            checked = b.check()
            few = max(calls // 5, 4)
            us = timed(torch, [("verify_b", b.verify_batched, calls), ("verify_l", b.verify_loop, few),
                               ("refine_b", b.refine_batched, calls), ("refine_l", b.refine_loop, few)], passes)
            out[f"{model}_P{P}"] = {
                "checked": checked, "stream_us": us,
                "verify_loop_over_batched": round(us["verify_l"]["median"] / us["verify_b"]["median"], 2),
                "refine_loop_over_batched": round(us["refine_l"]["median"] / us["refine_b"]["median"], 2),
                "verify_batched_wholly_below_loop": bool(us["verify_b"]["max"] < us["verify_l"]["min"]),
                "refine_batched_wholly_below_loop": bool(us["refine_b"]["max"] < us["refine_l"]["min"])}
            print(f"batched {model} P = {P}: {out[f'{model}_P{P}']['verify_loop_over_batched']} "
                  f"{out[f'{model}_P{P}']['refine_loop_over_batched']}", file=sys.stderr, flush=True)
            del b
    return out


def child(calls):
    """The calls that existed before, alone, on this process's library: verify_device, verify_homography_device and one
    refine_homography_device round at K = 1024."""
    import torch

    f, h = vb.Legs(), Single("h")
    f.check(K_REFIT)
    h.check(K_REFIT)
    h.check_refit()
    legs = [("verify_device", lambda: f.verify(K_REFIT), calls),
            ("verify_homography_device", lambda: h.verify(K_REFIT), calls),
            ("refine_homography_device", lambda: h.refine(1), calls)]
    for _ in range(20):
        for _, fn, _c in legs:
            fn()
    us = timed(torch, legs, 5)
    out = {"library": sift.version()}
    out.update({k: v["median"] for k, v in us.items()})
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
                raise SystemExit(f"existing-calls child ({name}) failed: {r.stdout[-500:]}{r.stderr[-500:]}")
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-batched", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine", "verify_affine_bench.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verify_affine_bench needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    res = {"workload": f"{N} matches ({N_IN} pairs planted under an affine map (a), a similarity (s) or a plane's "
                       f"homography (h) + {N - N_IN} pairs of unrelated positions, {W} x {H}), max_error {MAX_ERROR}, seed 0 "
                       f"(pair p of a batch: seed p); stream_us: back-to-back calls between HIP events, per call",
           "library": sift.version(), "passes": a.passes, "calls_per_pass": a.calls,
           "not_measured": "occupancy or any other counter, a kernel trace, the chain with the matcher, more than one GPU, "
                           "the C++ surface"}
    res["single"], res["refit"] = single(a.passes, a.calls)
    if not a.no_batched:
        res["batched"] = batched(a.passes, max(a.calls // 2, 4))
    if a.parent_lib:
        res["existing_calls_vs_parent"] = parent_pairs(os.path.abspath(a.parent_lib), a.passes, a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
