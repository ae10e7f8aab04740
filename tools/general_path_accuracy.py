"""The matcher's general (fp16) path against the float64 reference, as figures: profiles/general_path/accuracy.json.

    python3 tools/general_path_accuracy.py [--build this] [--out profiles/general_path/accuracy.json]

The inputs, the reference and the rules are those of tests/general_cases.py and the routes those of
tests/test_gpu_match_general.py (whose assertions are the contract; nothing is asserted here, so a build that breaks
it -- SIFT_HIP_LIB pointing at a library of the parent commit -- is measured all the same).  Per family, direction and
route: the maximum and median of |d2_gpu - D|, the maximum of |err| / B, the number of negative and NaN d2, the
decidable share of the queries, the number of undecidable queries whose indices differ from the float64 order, and
the number of rows that break each rule.  `duplicates` holds what the planted duplicate queries 0, 1 and 2 got.  The
figures of a build are merged into --out under its --build name.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "another-cuda-sift_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import general_cases as gc  # noqa: E402
import sift_amd as sift  # noqa: E402
import test_gpu_match_general as tg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_path", "accuracy.json"))
    a = ap.parse_args()
    if sift.device_count() < 1:
        raise SystemExit("general_path_accuracy needs a GPU: nothing is measured without one")
    res = {"library": sift.version(), "shape": [gc.NQ, gc.NT], "bound": "136 * 2^-23 * (|q|^2 + |t|^2 + 2 sum |q_k||t_k|)",
           "families": {}}
    for family in gc.FAMILIES:
        c = gc.case(family)
        _, out = tg.runs(sift, family)
        fam = res["families"][family] = {}
        for dn in ("fwd", "rev"):
            d = getattr(c, dn)
            fam[dn] = {}
            for route, (idx2, d2, _) in out[dn].items():
                g = tg.GATE_OF[route]
                stats, bad = gc.measure_top2(idx2, d2, d.D, d.B, d.cand[g], d.ref[g])
                stats["rows_breaking"] = {k: int(len(v)) for k, v in bad.items() if len(v)}
                fam[dn][route] = stats
        fam["duplicates"] = {route: {f"query_{q}": {"idx2": idx2[q].tolist(), "d2": [float(x) for x in d2[q]],
                                                    "match": int(match[q])} for q in (0, 1, 2)}
                             for route, (idx2, d2, match) in out["fwd"].items()}
    try:
        allres = json.load(open(a.out))
    except (OSError, ValueError):
        allres = {}
    allres[a.build] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(allres, f, indent=1)
        f.write("\n")
    worst = max(s["max_err_over_B"] for fam in res["families"].values() for dn in ("fwd", "rev") for s in fam[dn].values())
    neg = sum(s["negative_d2"] for fam in res["families"].values() for dn in ("fwd", "rev") for s in fam[dn].values())
    print(f"{a.build}: {res['library']}: max |err| / B {worst:.4f}, negative d2 {neg}; written to {a.out}")


if __name__ == "__main__":
    main()
