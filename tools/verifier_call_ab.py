#!/usr/bin/env python3
"""The host share of a verifier call, this build against another build of the library (normally the parent commit's).

    python3 tools/verifier_call_ab.py --parent-lib <other build's libsift_hip.so> [--passes 5]

Both libraries are driven by this tree's Python package (the C ABI is the same) in separate processes, alternating
other / this `--passes` times.  Each process measures, on the lists of tools/verify_refit_bench.py (2000 matches,
K = 1024; `Single`) and of tools/verify_batched_bench.py at P = 7 (`Refined`), for both models:

  enqueue_*   the device forms: wall-clock per call of a burst of calls that only enqueue (the stream is synchronised
              after the burst, outside the clock) -- the host path of verify_device, refine_device and their batched forms
  host_*      the synchronous host forms, wall-clock per call: verify_host, refine_host and their batched forms

and reports the median over its bursts; the parent process collects the medians of the passes, their range per build,
and whether the two ranges overlap.  `digest` is a hash of what the host forms returned: equal in every process.
"""
import argparse
import hashlib
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

BURSTS, P = 9, 7


def child(calls):
    import torch

    import verify_refit_bench as vrb

    K, E = vrb.K, vrb.MAX_ERROR
    legs, digest = [], hashlib.sha1()
    keep = []
    for model in "fh":
        s, b = vrb.Single(model), vrb.Refined(model, P)
        keep += [s, b]
        b.prepare()
        host = (s.v.verify_homography_host, s.v.refine_homography_host, b.v.verify_homography_batched_host,
                b.v.refine_homography_batched_host) if model == "h" else (s.v.verify_host, s.v.refine_host,
                                                                          b.v.verify_batched_host,
                                                                          b.v.refine_batched_host)
        rec, _recs, mask = host[0](*s.args, E, K, 0, 2, 2, True)
        verified = host[2](b.dm.data_ptr(), 0, b.pairs, E, K, 0, 2, 2, True)
        for got in (host[0](*s.args, E, K, 0, 2, 2, True), host[1](*s.args, rec, mask, E, 1, 2, 2)):
            for x in got[:3]:
                digest.update(np.asarray(x).tobytes())
        for got in (verified, host[3](b.dm.data_ptr(), 0, b.pairs, verified, E, 1, 2, 2)):
            for pair in got:
                for x in pair[:3]:
                    digest.update(np.asarray(x).tobytes())
        legs += [
            (f"enqueue_verify_{model}", s.verify, True),
            (f"enqueue_refine_{model}", lambda s=s: s.refine(1), True),
            (f"enqueue_verify_batched_{model}", lambda b=b: b.batched(K), True),
            (f"enqueue_refine_batched_{model}", lambda b=b: b.refine_batched(1), True),
            (f"host_verify_{model}", lambda s=s, f=host[0]: f(*s.args, E, K, 0, 2, 2, True), False),
            (f"host_refine_{model}", lambda s=s, f=host[1], r=rec, m=mask: f(*s.args, r, m, E, 1, 2, 2), False),
            (f"host_verify_batched_{model}", lambda b=b, f=host[2]: f(b.dm.data_ptr(), 0, b.pairs, E, K, 0, 2, 2, True),
             False),
            (f"host_refine_batched_{model}",
             lambda b=b, f=host[3], v=verified: f(b.dm.data_ptr(), 0, b.pairs, v, E, 1, 2, 2), False),
        ]
    for _, fn, _e in legs:
        for _ in range(5):
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
    out = {"library": sift.version(), "digest": digest.hexdigest(),
           "us": {k: round(float(np.median(v)), 3) for k, v in t.items()}}
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_call", "host_ab.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("verifier_call_ab needs a GPU: nothing is measured without one")
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
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls)], env=env,
                               capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode or not line:
                raise SystemExit(f"child ({name}, pass {i}) failed ({r.returncode}): {r.stdout[-500:]}{r.stderr[-1500:]}")
            rows[name].append(json.loads(line[-1][6:]))
            print(f"pass {i} {name}: {line[-1][6:]}", file=sys.stderr, flush=True)
    digests = {r["digest"] for rs in rows.values() for r in rs}
    res = {"what": f"wall-clock us per call, median of {BURSTS} bursts of {a.calls} calls per process; {a.passes} "
                   f"processes per build, alternating parent / new on one GPU; single lists: 2000 matches, K = 1024; "
                   f"batches: P = {P} such lists; refine: 1 round",
           "libraries": {k: v[0]["library"] for k, v in rows.items()},
           "host_form_outputs_equal_in_every_process": len(digests) == 1, "legs": {}}
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


if __name__ == "__main__":
    main()
