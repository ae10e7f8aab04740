#!/usr/bin/env python3
"""The matcher's host path, this build against another build of the library (normally the parent commit's): the same
bytes out of every match entry point over every route, and the host time of a call.

    python3 tools/matcher_call_ab.py --parent-lib <other build's libsift_hip.so> [--passes 5]

Both libraries are driven by this tree's Python package (the C ABI is the same) in fresh child processes, alternating
other / this `--passes` times; a child that fails or runs out of its time ends the run.  Each child

  digest      calls every match entry point (top-2, list, k-NN table, k-NN list; plain, window, epipolar; single pair,
              batch, ready codes; device and host forms) over the routes of the host path -- a pair of detector
              buffers (sidecars), a foreign single pair, prepared batches of P = 1, 3 and 33 pairs on a matcher of
              max_pairs = 40 (33 crosses the 32-pair cut of a gated launch; a cross check takes the one-pass reverse
              at P = 3 and the two-pass reverse at P = 33), ready code sets, and pairs with a set that holds a
              non-integer value (the fp16 path) -- with nq = 300 and nt = 700 (more than one 256-query block, 256-row
              key group and split), a pair with nt = 0, a pair with nq = 0 and sets shared between pairs, k in 1, 4, 5,
              8, and hashes every output buffer after every call: equal in every process of both builds.
  enqueue_*   the device forms: wall-clock per call of a burst of calls that only enqueue (the stream is synchronised
              after the burst, outside the clock).
  host_*      the synchronous host forms, wall-clock per call.

and reports the median over its bursts; the parent process collects the medians of the passes, their range per build,
and whether the two ranges overlap.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "another-cuda-sift_amd"))
import sift_amd as sift  # noqa: E402

BURSTS, NQ, NT, MAX_PAIRS = 9, 300, 700, 40
OPS = {"top2": "", "list": "list_", "knn": "knn_", "knn_list": "knn_list_"}
GATES = {"none": "", "window": "guided_", "epipolar": "epipolar_"}
SINGLE = [(op, g, "single", "device") for op in OPS for g in GATES]
BATCHED = [(op, g, "batched", "device") for op in OPS for g in GATES]
HOST = [(op, g, "single", "host") for op in OPS for g in GATES if op != "top2" or g == "none"]
CODES = [(op, "none", "codes", "device") for op in ("top2", "list", "knn")] + [("list", g, "codes", "device")
                                                                               for g in ("window", "epipolar")]
F = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)  # the epipolar lines are the rows: |y_train - y_query| <= max_error
RADIUS, MAX_ERROR = 60.0, 10.0
FILTERS = (dict(ratio=0.8, cross_check=1), dict(ratio=0.9, ratio_both_ways=1, cross_check=0),
           dict(ratio=0.8, cross_check=0))


def entry_name(e):
    op, gate, shape, form = e
    return f"sift_hip_match_{OPS[op]}{GATES[gate]}{'codes_' if shape == 'codes' else ''}" \
           f"{form if shape == 'single' else 'batched'}"


class World:
    """The sets, the outputs and the matcher of one child."""

    def __init__(self, torch):
        self.torch = torch
        rng = np.random.default_rng(11)
        w, h = 752, 480
        self.det = sift.Detector(sift.CudaSiftConfig(col_width=w, row_width=h, numFeatures=2000), lanes=1)
        self.det.gpuWarmUpAndAllocate()
        for f in (30, 31):
            self.det.detectAndCompute(sift.synth_frame(f, w, h))
        torch.cuda.synchronize()
        n0, n1 = min(self.det.prev_size, NQ), min(self.det.total_size, NT)
        assert n0 == NQ and n1 > 256, (n0, n1)

        def xy(n):
            return torch.from_numpy(rng.uniform(0.0, 100.0, (n, 2)).astype(np.float32)).cuda()

        # name -> (rows pointer, rows, positions); P and Q are the detector's buffers (fresh sidecars), G holds a 0.5
        self.sets, self.keep, codes, keys, self.row0, at = {}, [], [], [], {}, 0
        self.sets["P"] = (self.det.prev_descriptor.data(), n0, xy(n0))
        self.sets["Q"] = (self.det.device_descriptor.data(), n1, xy(n1))
        for name in "ABCG":
            a = rng.integers(0, 256, (NT, 128)).astype(np.float16)
            if name == "G":
                a[NQ // 2, 5] = 0.5
            rows = torch.from_numpy(a.view(np.int16)).cuda()
            self.keep.append(rows)
            self.sets[name] = (rows.data_ptr(), NT, xy(NT))
            if name != "G":
                from sift_amd import multi

                c, k = multi.codes_from_rows(rows)
                codes.append(c), keys.append(k)
                self.row0[name], at = at, at + NT
        self.codes, self.keys = torch.cat(codes).contiguous(), torch.cat(keys).contiguous()
        self.geometry = torch.tensor(F * MAX_PAIRS, dtype=torch.float32, device="cuda")
        rows = 33 * NQ
        self.idx = torch.empty(rows * 8, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(rows * 8, dtype=torch.float32, device="cuda")
        self.match = torch.empty(rows, dtype=torch.int32, device="cuda")
        self.out = torch.empty(rows * 8 * 4, dtype=torch.int32, device="cuda")
        self.counts = torch.empty(64, dtype=torch.int32, device="cuda")
        self.matcher = sift.Matcher(NT, NT, MAX_PAIRS)
        self.L = sift.lib()
        torch.cuda.synchronize()

    def call(self, e, pairs, k=4, flt=FILTERS[0]):
        """(run, outputs): run() makes the call of entry point e on pairs [(query set, nq, train set, nt)];
        outputs() are the bytes it left."""
        op, gate, shape, form = e
        fn = getattr(self.L, entry_name(e))
        P, m, keep = len(pairs), self.matcher._m, []
        ints = lambda v: (ctypes.c_int * len(v))(*v)  # noqa: E731
        nq, nt = [p[1] for p in pairs], [p[3] for p in pairs]
        if shape == "single":
            (qs, _, ts, _), = pairs
            head = [m, self.sets[qs][0], nq[0], self.sets[ts][0], nt[0]]
            if gate == "window":
                g = sift._MatchGate(self.sets[qs][2].data_ptr(), 2, self.sets[ts][2].data_ptr(), 2, RADIUS)
            elif gate == "epipolar":
                g = sift._MatchEpipolarGate(self.sets[qs][2].data_ptr(), 2, self.sets[ts][2].data_ptr(), 2, RADIUS,
                                            (ctypes.c_float * 9)(*F), MAX_ERROR)
            if gate != "none":
                keep.append(g)
                head.append(ctypes.pointer(g))
        else:
            if shape == "batched":
                head = [m, P, (ctypes.c_void_p * P)(*[self.sets[p[0]][0] for p in pairs]), ints(nq),
                        (ctypes.c_void_p * P)(*[self.sets[p[2]][0] for p in pairs]), ints(nt)]
            else:
                q0, t0 = ints([self.row0[p[0]] for p in pairs]), ints([self.row0[p[2]] for p in pairs])
                head = [m, self.codes.data_ptr(), self.keys.data_ptr(), P, q0, q0, ints(nq), t0, t0, ints(nt)]
            if gate != "none":
                head += [(sift._MatchPositions * P)(*[sift._MatchPositions(self.sets[p[0]][2].data_ptr(),
                                                                           self.sets[p[2]][2].data_ptr()) for p in pairs]),
                         2, 2, RADIUS]
                if gate == "epipolar":
                    head += [self.geometry.data_ptr(), 36, MAX_ERROR]
        f = sift._MatchFilter(flt.get("ratio", 0.8), 0, flt.get("ratio_both_ways", 0), flt.get("max_distance", 0.0),
                              flt["cross_check"])
        keep.append(f)
        n = nq[0] * (k if op.startswith("knn") else 1)
        hidx, hd2 = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.float32)
        hrec, hcount = np.full((max(n, 1), 4), -7, np.int32), ctypes.c_int(-7)
        dev = form == "device"
        if op == "top2":
            tail = [0.8, 0, self.idx.data_ptr(), self.d2.data_ptr(), self.match.data_ptr(), None] if dev \
                else [0.8, 0, hidx.ctypes.data]
        elif op == "list":
            tail = [ctypes.pointer(f)] + ([self.out.data_ptr(), self.counts.data_ptr(), None] if dev
                                          else [hrec.ctypes.data, n, ctypes.byref(hcount)])
        elif op == "knn":
            tail = [k] + ([self.idx.data_ptr(), self.d2.data_ptr(), None] if dev else [hidx.ctypes.data, hd2.ctypes.data])
        else:
            tail = [k, 1.0e6] + ([self.out.data_ptr(), self.counts.data_ptr(), None] if dev
                                 else [hrec.ctypes.data, n, ctypes.byref(hcount)])
        args = [ctypes.cast(ctypes.c_void_p(x), ty) if isinstance(x, int) and hasattr(ty, "contents") else x
                for x, ty in zip(head + tail, fn.argtypes)]
        assert len(args) == len(fn.argtypes), entry_name(e)

        def run():
            rc = fn(*args)
            if rc:
                raise SystemExit(f"{entry_name(e)} {pairs}: {rc} {self.L.sift_hip_last_error().decode()}")

        def outputs():
            if dev:
                self.torch.cuda.synchronize()
                return [x.cpu().numpy().tobytes() for x in (self.idx, self.d2, self.match, self.out, self.counts)]
            return [hidx.tobytes(), hd2.tobytes(), hrec.tobytes(), bytes(ctypes.c_int(hcount.value))]

        run.keep = keep + [hidx, hd2, hrec, hcount]  # the host outputs live as long as the call does
        return run, outputs

    def clear(self):
        for x in (self.idx, self.match, self.out, self.counts):
            x.fill_(-7)
        self.d2.fill_(-7.0)


KINDS = [("A", NQ, "B", NT), ("A", NQ, "B", 0), ("A", 0, "B", NT), ("C", NQ, "B", NT), ("G", NQ, "A", NQ)]


def tables(general):
    """The pair tables of the batched forms: P = 1, 3 (a plain pair, one without train rows, one without query rows:
    A and B are shared) and 33 (those, a pair sharing B, and with `general` a pair whose query set is not integers)."""
    kinds = KINDS if general else KINDS[:4]
    return [kinds[:1], kinds[:3], [kinds[i % len(kinds)] for i in range(33)]] + ([kinds[2:5]] if general else [])


def variants(e):
    if e[0] == "list":
        return [dict(flt=f) for f in FILTERS]
    if e[0] in ("knn", "knn_list"):
        return [dict(k=k) for k in (1, 4, 5, 8)]
    return [{}]


def digest_all(w):
    h, calls = hashlib.sha1(), 0
    work = [(e, [pair]) for e in SINGLE + HOST
            for pair in (("P", NQ, "Q", w.sets["Q"][1]), ("Q", 257, "P", NQ - 3), ("A", NQ, "B", NT), ("G", NQ, "B", NT),
                         ("A", NQ, "A", NT), ("A", NQ, "B", 0), ("A", 0, "B", NT))]
    work += [(e, t) for e in BATCHED for t in tables(True)] + [(e, t) for e in CODES for t in tables(False)]
    for e, pairs in work:
        for v in variants(e):
            run, outputs = w.call(e, pairs, **v)
            w.clear()
            run()
            for b in outputs():
                h.update(b)
            calls += 1
    return h.hexdigest(), calls


def child(calls):
    import faulthandler

    import torch

    faulthandler.enable()
    w = World(torch)
    print("child: sets ready", file=sys.stderr, flush=True)
    digest, ncalls = digest_all(w)
    print(f"child: digest of {ncalls} calls", file=sys.stderr, flush=True)
    one, three, many = tables(False)[:3]
    legs = [(f"enqueue_{entry_name(e)[15:]}_sidecars", w.call(e, [("P", NQ, "Q", w.sets["Q"][1])])[0], True) for e in SINGLE]
    legs += [(f"enqueue_{entry_name(e)[15:]}", w.call(e, one)[0], True) for e in SINGLE]
    legs += [(f"enqueue_{entry_name(e)[15:]}_P{len(t)}", w.call(e, t)[0], True) for e in BATCHED + CODES for t in (three, many)]
    legs += [(f"host_{entry_name(e)[15:]}", w.call(e, one)[0], False) for e in HOST]
    for _, fn, _e in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k, _, _ in legs}
    for _ in range(BURSTS):
        for k, fn, _e in legs:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[k].append((time.perf_counter() - t0) / calls * 1e6)
            torch.cuda.synchronize()
    out = {"library": sift.version(), "digest": digest, "digest_calls": ncalls,
           "us": {k: round(float(np.median(v)), 3) for k, v in t.items()}}
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matcher_call", "host_ab.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("matcher_call_ab needs a GPU: nothing is measured without one")
    if a.child:
        child(a.calls)
        return
    if not a.parent_lib:
        raise SystemExit("--parent-lib: the other build's libsift_hip.so")
    rows = {"parent": [], "new": []}
    for i in range(a.passes):
        for name, libpath in (("parent", os.path.abspath(a.parent_lib)), ("new", None)):
            env = dict(os.environ)
            env.pop("SIFT_HIP_LIB", None)
            if libpath:
                env["SIFT_HIP_LIB"] = libpath
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], env=env,
                                   capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"child ({name}, pass {i}) ran out of its {a.child_timeout} s: stopping")
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode or not line:
                raise SystemExit(f"child ({name}, pass {i}) failed ({r.returncode}): {r.stdout[-500:]}{r.stderr[-1500:]}")
            rows[name].append(json.loads(line[-1][6:]))
            print(f"pass {i} {name}: digest {rows[name][-1]['digest']} ({rows[name][-1]['digest_calls']} calls)",
                  file=sys.stderr, flush=True)
    digests = {r["digest"] for rs in rows.values() for r in rs}
    res = {"what": f"wall-clock us per call, median of {BURSTS} bursts of {a.calls} calls per process; {a.passes} "
                   f"processes per build, alternating parent / new on one GPU; pairs of {NQ} x {NT} rows, P3 / P33: "
                   f"batches of 3 / 33 pairs on a matcher of max_pairs = {MAX_PAIRS}; k = 4; the default filter",
           "libraries": {k: v[0]["library"] for k, v in rows.items()},
           "digest": sorted(digests), "digest_calls": rows["new"][0]["digest_calls"],
           "outputs_equal_in_every_process": len(digests) == 1, "legs": {}}
    for leg in rows["new"][0]["us"]:
        e = {}
        for name in ("parent", "new"):
            v = [r["us"][leg] for r in rows[name]]
            e[name] = {"pass_medians": v, "median": round(float(np.median(v)), 3), "min": min(v), "max": max(v)}
        e["ranges_overlap"] = bool(e["new"]["min"] <= e["parent"]["max"] and e["parent"]["min"] <= e["new"]["max"])
        e["new_over_parent"] = round(e["new"]["median"] / e["parent"]["median"], 4)
        res["legs"][leg] = e
    res["every_leg_overlaps"] = all(e["ranges_overlap"] for e in res["legs"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["parent"]["median"], v["new"]["median"], v["ranges_overlap"]) for k, v in res["legs"].items()}))
    print("every leg overlaps:", res["every_leg_overlaps"], "outputs equal:", len(digests) == 1)
    if len(digests) != 1:
        raise SystemExit("the builds' outputs differ")


if __name__ == "__main__":
    main()
