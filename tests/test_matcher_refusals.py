"""The matcher's refusals, pinned: status and exact message of every match entry point, without a GPU.

Every call runs on host memory that is never read or written, on a matcher that is null or a zeroed block standing in
for one (its leading ints are the handle's device, max_query, max_train and max_pairs; every pointer in it is null, so
it serves only calls that are refused), and breaks exactly one argument rule; the handle's own limits are met on
otherwise valid calls, on stand-ins whose limit fields are filled in so that exactly one of them refuses.  EXPECTED was
produced by running this table on the commit before the match entry points were given one call record and one checker,
and pasted in: a message that moves is a change of the documented surface.  ORDER pins what a call with two faults
reports -- the one order include/sift_hip.h states for the gated k-NN calls, which covers every family's rules -- and
that a single-pair entry point and its one-pair batch refuse by the same rule.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

INVALID = -1  # SIFT_HIP_ERR_INVALID
OPS = {"top2": "", "list": "list_", "knn": "knn_", "knn_list": "knn_list_"}
GATES = {"none": "", "window": "guided_", "epipolar": "epipolar_"}
# (operation, gate, shape: single | batched | codes, form: device | host); the codes forms are batches of ready code sets.
ENTRIES = ([(op, g, "single", "device") for op in OPS for g in GATES]
           + [(op, g, "batched", "device") for op in OPS for g in GATES]
           + [(op, g, "single", "host") for op in OPS for g in GATES if (op, g) not in (("top2", "window"),
                                                                                          ("top2", "epipolar"))]
           + [(op, "none", "codes", "device") for op in ("top2", "list", "knn")]
           + [("list", g, "codes", "device") for g in ("window", "epipolar")])
LIMITS_OK = (8, 8, 4)  # max_query, max_train, max_pairs of the stand-in the one-fault calls run on
GOOD = dict(P=2, nq=4, nt=4, q=True, t=True, nq_arr=True, nt_arr=True, q_arr=True, t_arr=True, codes=True, keys=True,
            qrow0_arr=True, tkey0_arr=True, qrow0=0, tkey0=0, gate=True, positions=True, qxy=True, txy=True, qs=2, ts=2,
            radius=5.0, max_error=1.5, F=(0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0), geometry=True, gstride=36,
            filter=True, k=2, maxd=1.0, out=True, counts=True, cap=4)


def batch(e):
    return e[2] != "single"


def gated(e):
    return e[1] != "none"


def fp16(e):
    return e[2] != "codes"


def lists(e):
    return e[0] in ("list", "knn_list")


# One broken rule each; `on` says which entry points have the rule.  A fault of one pair is the last pair's in a batch.
FAULTS = {
    "k_0": (dict(k=0), lambda e: e[0] in ("knn", "knn_list")),
    "k_9": (dict(k=9), lambda e: e[0] in ("knn", "knn_list")),
    "maxd_nan": (dict(maxd=math.nan), lambda e: e[0] == "knn_list"),
    "null_gate": (dict(gate=False), lambda e: gated(e) and not batch(e)),
    "qstride_1": (dict(qs=1), gated),
    "tstride_1": (dict(ts=1), gated),
    "radius_0": (dict(radius=0.0), gated),
    "radius_nan": (dict(radius=math.nan), gated),
    "max_error_0": (dict(max_error=0.0), lambda e: e[1] == "epipolar"),
    "max_error_inf": (dict(max_error=math.inf), lambda e: e[1] == "epipolar"),
    "F_nan": (dict(F=(1.0, 0.0, math.nan) + (0.0,) * 6), lambda e: e[1] == "epipolar" and not batch(e)),
    "F_zero": (dict(F=(0.0,) * 9), lambda e: e[1] == "epipolar" and not batch(e)),
    "null_geometry": (dict(geometry=False), lambda e: e[1] == "epipolar" and batch(e)),
    "gstride_32": (dict(gstride=32), lambda e: e[1] == "epipolar" and batch(e)),
    "gstride_38": (dict(gstride=38), lambda e: e[1] == "epipolar" and batch(e)),
    "P_0": (dict(P=0), batch),
    "P_5": (dict(P=5), batch),
    "null_nq": (dict(nq_arr=False), batch),
    "null_nt": (dict(nt_arr=False), batch),
    "null_positions": (dict(positions=False), lambda e: gated(e) and batch(e)),
    "null_filter": (dict(filter=False), lambda e: e[0] == "list"),
    "null_q_array": (dict(q_arr=False), lambda e: e[2] == "batched"),
    "null_t_array": (dict(t_arr=False), lambda e: e[2] == "batched"),
    "null_codes": (dict(codes=False), lambda e: e[2] == "codes"),
    "null_keys": (dict(keys=False), lambda e: e[2] == "codes"),
    "null_qrow0": (dict(qrow0_arr=False), lambda e: e[2] == "codes"),
    "null_tkey0": (dict(tkey0_arr=False), lambda e: e[2] == "codes"),
    "nq_neg": (dict(nq=-1), lambda e: True),
    "nt_neg": (dict(nt=-1), lambda e: True),
    "nq_9": (dict(nq=9), lambda e: True),
    "nt_9": (dict(nt=9), lambda e: True),
    "null_q": (dict(q=False), fp16),
    "null_t": (dict(t=False), fp16),
    "neg_qrow0": (dict(qrow0=-1), lambda e: e[2] == "codes"),
    "neg_tkey0": (dict(tkey0=-1), lambda e: e[2] == "codes"),
    "null_qxy": (dict(qxy=False), gated),
    "null_txy": (dict(txy=False), gated),
    "null_out": (dict(out=False), lambda e: lists(e) or e == ("top2", "none", "single", "host")),
    "null_counts": (dict(counts=False), lists),
    "cap_neg": (dict(cap=-1), lambda e: lists(e) and e[3] == "host"),
}
# The handle's limits on a valid call of pairs of 4 x 6 rows (a batch: 2 pairs): the stand-in's (max_query, max_train,
# max_pairs), of which exactly one is too small; the reverse pair's limit is met by the list calls only (the filter
# asks for a cross check).
LIMITS = {
    "over_max_query": ((3, 8, 4), lambda e: True),
    "over_max_train": ((8, 5, 4), lambda e: True),
    "over_max_pairs": ((8, 8, 1), batch),
    "reverse_over_max_query": ((4, 8, 4), lambda e: e[0] == "list"),
}


def entry_name(e):
    op, gate, shape, form = e
    return f"sift_hip_match_{OPS[op]}{GATES[gate]}{'codes_' if shape == 'codes' else ''}" \
           f"{form if shape == 'single' else 'batched'}"


def short(e):
    return entry_name(e)[len("sift_hip_match_"):]


class Calls:
    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(1024, np.int32)  # every output and every set: never read, never written
        self.fake = np.zeros(64, np.int64)

    def stand_in(self, limits):
        self.fake[:] = 0
        self.fake.view(np.int32)[1:4] = limits
        return self.fake.ctypes.data

    def run(self, e, m, **faults):
        a = dict(GOOD, **faults)
        op, gate, shape, form = e
        fn = getattr(self.L, entry_name(e))
        p = self.buf.ctypes.data
        ptr = lambda on, off=0: p + off if on else None  # noqa: E731
        ints = lambda on, v: (ctypes.c_int * len(v))(*v) if on else None  # noqa: E731
        q, t, qxy, txy = ptr(a["q"]), ptr(a["t"], 512), ptr(a["qxy"], 1024), ptr(a["txy"], 1536)
        keep = []
        if shape == "single":
            head = [m, q, a["nq"], t, a["nt"]]
        else:
            n = max(min(a["P"], 8), 1)
            nq, nt = ints(a["nq_arr"], [4] * (n - 1) + [a["nq"]]), ints(a["nt_arr"], [4] * (n - 1) + [a["nt"]])
            if shape == "batched":
                qa = (ctypes.c_void_p * n)(*([p] * (n - 1) + [q])) if a["q_arr"] else None
                ta = (ctypes.c_void_p * n)(*([p + 512] * (n - 1) + [t])) if a["t_arr"] else None
                head = [m, a["P"], qa, nq, ta, nt]
            else:
                zeros = ints(True, [0] * n)
                head = [m, ptr(a["codes"]), ptr(a["keys"], 512), a["P"], ints(a["qrow0_arr"], [0] * (n - 1) + [a["qrow0"]]),
                        zeros, nq, zeros, ints(a["tkey0_arr"], [0] * (n - 1) + [a["tkey0"]]), nt]
            if gate != "none":
                pos = (self.sift._MatchPositions * n)(*([self.sift._MatchPositions(p + 1024, p + 1536)] * (n - 1)
                                                        + [self.sift._MatchPositions(qxy, txy)]))
                head += [pos if a["positions"] else None, a["qs"], a["ts"], a["radius"]]
                if gate == "epipolar":
                    head += [ptr(a["geometry"], 2048), a["gstride"], a["max_error"]]
        if gate != "none" and shape == "single":
            if gate == "window":
                g = self.sift._MatchGate(qxy, a["qs"], txy, a["ts"], a["radius"])
            else:
                g = self.sift._MatchEpipolarGate(qxy, a["qs"], txy, a["ts"], a["radius"], (ctypes.c_float * 9)(*a["F"]),
                                                 a["max_error"])
            keep.append(g)
            head.append(ctypes.pointer(g) if a["gate"] else None)
        flt = self.sift._MatchFilter(0.8, 0, 0, 0.0, 1)
        out, counts = ptr(a["out"], 2560), ptr(a["counts"], 3072)
        if op == "top2":
            tail = [0.8, 0, None, None, out, None] if form == "device" else [0.8, 0, out]
        elif op == "list":
            tail = [ctypes.pointer(flt) if a["filter"] else None, out] + ([counts, None] if form == "device"
                                                                           else [a["cap"], counts])
        elif op == "knn":
            tail = [a["k"], out, counts] + ([None] if form == "device" else [])
        else:
            tail = [a["k"], a["maxd"], out] + ([counts, None] if form == "device" else [a["cap"], counts])
        args = [ctypes.cast(ctypes.c_void_p(x), ty) if isinstance(x, int) and hasattr(ty, "contents") else x
                for x, ty in zip(head + tail, fn.argtypes)]
        assert len(args) == len(fn.argtypes), entry_name(e)
        before = self.fake.copy()
        rc = fn(*args)
        msg = self.L.sift_hip_last_error().decode() if rc else ""
        assert not self.buf.any() and np.array_equal(self.fake, before), "a refused call wrote host memory"
        return rc, msg


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


def table(calls):
    """Every (entry point, case) of the pinned table -> (status, message)."""
    got = {}
    for e in ENTRIES:
        got[f"{short(e)} null_matcher"] = calls.run(e, None)
        for fault, (kw, on) in FAULTS.items():
            if on(e):
                got[f"{short(e)} {fault}"] = calls.run(e, calls.stand_in(LIMITS_OK), **kw)
        for limit, (limits, on) in LIMITS.items():
            if on(e):
                got[f"{short(e)} {limit}"] = calls.run(e, calls.stand_in(limits), nt=6)
    return got


# case -> [(message, which entry points report it)], the first selector that holds; the status is
# SIFT_HIP_ERR_INVALID, except where the message is "" (the call is accepted: status 0; sift_hip_match_host returns
# before it looks at an nq <= 0).  Twenty-two rows -- the set arrays, set pointers and set rows of the four gated list
# batches, and the set pointers of sift_hip_match_list_host -- were judged after the first list call's allocation on
# that commit, which fails first on a machine without a GPU; their rows are the messages its code states.
def knn(e):
    return e[0] in ("knn", "knn_list")


def epipolar(e):
    return e[1] == "epipolar"


def host(e):
    return e[3] == "host"


def plain(op):
    return lambda e: e[0] == op and e[1] == "none"


def everyone(e):
    return True


TOP2_CODES = lambda e: e == ("top2", "none", "codes", "device")  # noqa: E731
GATE = lambda msg: [("epipolar gate: " + msg, epipolar), ("match gate: " + msg, everyone)]  # noqa: E731
PAIRS = lambda knn_msg: [("bad gated batch", gated), (knn_msg, knn), ("bad code batch", TOP2_CODES),  # noqa: E731
                         ("bad batch", plain("top2")), ("bad match list arguments", everyone)]
SIZE = [("pair size exceeds matcher limits", everyone)]
OUTPUT = [("null argument", lambda e: host(e) and e[0] in ("top2", "list")),
          ("k-NN list: null out or count", lambda e: e[0] == "knn_list"), ("bad match list arguments", everyone)]
MAX_ERROR = [("epipolar gate: max_error must be > 0 and finite", everyone)]
GSTRIDE = [("epipolar gate: geometry_stride_bytes must be >= 36 and a multiple of 4", everyone)]
K = [("k-NN: k outside 1..SIFT_HIP_KNN_MAX", everyone)]
SET_ARRAY = [("k-NN: null descriptor array", knn), ("bad gated batch", gated), ("bad batch", plain("top2")),
             ("bad match list arguments", everyone)]
EXPECTED = {
    "null_matcher": [("null argument", lambda e: host(e) and e[1] == "none" and e[0] in ("top2", "list")),
                     ("bad code batch", TOP2_CODES), ("bad batch", plain("top2")),
                     ("bad match list arguments", plain("list")), ("null matcher", everyone)],
    "k_0": K,
    "k_9": K,
    "maxd_nan": [("k-NN list: max_distance is NaN", everyone)],
    "null_gate": [("null epipolar gate", epipolar), ("null match gate", everyone)],
    "qstride_1": GATE("a position stride below 2 floats"),
    "tstride_1": GATE("a position stride below 2 floats"),
    "radius_0": GATE("the radius must be > 0"),
    "radius_nan": GATE("the radius must be > 0"),
    "max_error_0": MAX_ERROR,
    "max_error_inf": MAX_ERROR,
    "F_nan": [("epipolar gate: a non-finite entry of F", everyone)],
    "F_zero": [("epipolar gate: F is all zero", everyone)],
    "null_geometry": [("epipolar gate: null geometry", everyone)],
    "gstride_32": GSTRIDE,
    "gstride_38": GSTRIDE,
    "P_0": PAIRS("k-NN: P outside 1..max_pairs"),
    "P_5": PAIRS("k-NN: P outside 1..max_pairs"),
    "over_max_pairs": PAIRS("k-NN: P outside 1..max_pairs"),
    "null_nq": PAIRS("k-NN: null size array"),
    "null_nt": PAIRS("k-NN: null size array"),
    "null_positions": [("bad gated batch", everyone)],
    "null_filter": [("null argument", host), ("bad match list arguments", everyone)],
    "null_q_array": SET_ARRAY,
    "null_t_array": SET_ARRAY,
    "null_codes": [("bad code batch", everyone)],
    "null_keys": [("bad code batch", everyone)],
    "null_qrow0": [("bad code batch", everyone)],
    "null_tkey0": [("bad code batch", everyone)],
    "nq_neg": [("", lambda e: e == ("top2", "none", "single", "host"))] + SIZE,
    "nt_neg": SIZE,
    "nq_9": SIZE,
    "nt_9": SIZE,
    "over_max_query": SIZE,
    "over_max_train": SIZE,
    "reverse_over_max_query": [("the reverse pair (roles swapped) exceeds matcher limits", everyone)],
    "null_q": [("null descriptor pointer", everyone)],
    "null_t": [("null descriptor pointer", everyone)],
    "neg_qrow0": [("negative set row", everyone)],
    "neg_tkey0": [("negative set row", everyone)],
    "null_qxy": GATE("null position pointer"),
    "null_txy": GATE("null position pointer"),
    "null_out": OUTPUT,
    "null_counts": OUTPUT,
    "cap_neg": [("k-NN list: null out or count", lambda e: e[0] == "knn_list"), ("null argument", everyone)],
}


def test_refusals_are_the_pinned_ones(calls):
    got = table(calls)
    assert len(got) > 800 and {k.split(" ", 1)[1] for k in got} == set(EXPECTED)
    by_name = {short(e): e for e in ENTRIES}
    for key, (rc, msg) in got.items():
        name, case = key.split(" ", 1)
        want = next(m for m, who in EXPECTED[case] if who(by_name[name]))
        assert (rc, msg) == (INVALID if want else 0, want), key


# Two faults in one call: the rule reported is the first in the shared order -- what needs no matcher (k, a NaN
# max_distance, the gate's fields), the matcher, P and the arrays, the pairs' sizes, the pointers of non-empty sets
# (descriptors or code rows, then positions), the outputs -- whatever the entry point.
# (the faults, which entry points, the message or the case of EXPECTED whose message it is)
ORDER = [
    (("null_matcher", "k_0"), knn, "k_0"),
    (("null_matcher", "maxd_nan"), lambda e: e[0] == "knn_list", "maxd_nan"),
    (("null_matcher", "tstride_1"), gated, "tstride_1"),
    (("null_matcher", "gstride_38"), lambda e: epipolar(e) and batch(e), "gstride_38"),
    (("null_matcher", "F_zero"), lambda e: epipolar(e) and not batch(e), "F_zero"),
    (("k_9", "maxd_nan"), lambda e: e[0] == "knn_list", "k_9"),
    (("maxd_nan", "radius_0"), lambda e: e[0] == "knn_list" and gated(e), "maxd_nan"),
    (("k_0", "null_gate"), lambda e: knn(e) and gated(e) and not batch(e), "k_0"),
    (("radius_nan", "max_error_0"), epipolar, "radius_nan"),
    (("max_error_inf", "null_geometry"), lambda e: epipolar(e) and batch(e), "max_error_inf"),
    (("max_error_inf", "F_nan"), lambda e: epipolar(e) and not batch(e), "max_error_inf"),
    (("null_matcher", "nq_9"), lambda e: not (host(e) and e[0] == "top2"), "null_matcher"),
    (("P_5", "nq_9"), batch, "P_5"),
    (("P_0", "null_out"), lambda e: batch(e) and lists(e), "P_0"),
    (("null_nt", "null_q_array"), lambda e: e[2] == "batched", "null_nt"),
    (("null_positions", "null_q"), lambda e: e[2] == "batched" and gated(e), "null_positions"),
    (("null_filter", "nt_9"), lambda e: e[0] == "list" and not host(e), "null_filter"),
    (("null_t_array", "nq_neg"), lambda e: e[2] == "batched", "null_t_array"),
    (("null_keys", "nt_neg"), lambda e: e[2] == "codes", "null_keys"),
    (("nt_9", "null_q"), fp16, "nt_9"),
    (("nq_9", "null_txy"), gated, "nq_9"),
    (("nt_neg", "neg_qrow0"), lambda e: e[2] == "codes", "nt_neg"),
    (("null_t", "null_qxy"), lambda e: gated(e) and fp16(e), "null_t"),
    (("neg_tkey0", "null_txy"), lambda e: gated(e) and not fp16(e), "neg_tkey0"),
    (("null_q", "null_out"), lambda e: lists(e) and fp16(e) and not host(e), "null_q"),
    (("null_txy", "null_counts"), lambda e: lists(e) and gated(e) and not host(e), "null_txy"),
    (("nq_neg", "null_counts"), lambda e: lists(e) and not host(e), "nq_neg"),
]


@pytest.mark.parametrize("case", ORDER, ids=lambda c: "+".join(c[0]))
def test_two_faults_report_the_first_rule_of_the_shared_order(calls, case):
    faults, on, first = case
    kw = {k: v for f in faults if f != "null_matcher" for k, v in FAULTS[f][0].items()}
    m = None if "null_matcher" in faults else calls.stand_in(LIMITS_OK)
    seen = 0
    for e in ENTRIES:
        if not on(e) or not all(f == "null_matcher" or FAULTS[f][1](e) for f in faults):
            continue
        seen += 1
        want = next(msg for msg, who in EXPECTED[first] if who(e))
        assert calls.run(e, m, **kw) == (INVALID, want), short(e)
    assert seen


# A single-pair entry point and its one-pair batch refuse by the same rule: the same case of EXPECTED answers both
# (the wording of the matcher's and the arrays' rules aside, which a single-pair call cannot break), with one fault
# and with two.
SINGLE_AND_BATCH = [("k_9",), ("maxd_nan",), ("qstride_1",), ("radius_0",), ("max_error_0",), ("nq_9",), ("nt_neg",),
                    ("null_q",), ("null_t",), ("null_qxy",), ("null_txy",), ("null_filter",), ("null_out",),
                    ("null_counts",), ("k_0", "tstride_1"), ("nq_9", "null_t"), ("null_q", "null_txy"),
                    ("null_txy", "null_out"), ("radius_nan", "nt_9")]


@pytest.mark.parametrize("faults", SINGLE_AND_BATCH, ids="+".join)
def test_a_single_pair_call_and_its_one_pair_batch_refuse_by_the_same_rule(calls, faults):
    kw = {k: v for f in faults for k, v in FAULTS[f][0].items()}
    seen = 0
    for e in ENTRIES:
        op, gate, shape, form = e
        twin = (op, gate, "batched", "device")
        if shape != "single" or form != "device" or not all(FAULTS[f][1](e) and FAULTS[f][1](twin) for f in faults):
            continue
        seen += 1
        rc, msg = calls.run(e, calls.stand_in(LIMITS_OK), **kw)
        want = next(m for m, who in EXPECTED[faults[0]] if who(e))
        assert (rc, msg) == (INVALID, want), short(e)
        assert calls.run(twin, calls.stand_in(LIMITS_OK), P=1, **kw) == (rc, msg), short(twin)
    assert seen


def test_every_match_entry_point_is_in_the_table():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sift_hip.h")
    declared = set(re.findall(r"^int (sift_hip_match_\w+)\(", open(header).read(), re.M))
    assert {n for n in declared if not n.endswith("_plan")} == {entry_name(e) for e in ENTRIES}
