"""The verifier's refusals, pinned: status and exact message of the sixteen verify and refine entry points and the two
score entry points, without a GPU.

Every call runs on host memory that is never read or written, on a verifier that is null or a zeroed block standing in
for one (as tests/test_verify_abi.py does), and breaks exactly one argument rule that can be judged without the
handle; the handle's own limits (hypotheses, then pairs, then rows) are met on otherwise valid calls, on stand-ins
whose limit fields are filled in so that exactly one of them refuses.  EXPECTED was produced by running this table on
the commit before the single and the batched host paths were merged, and pasted in: a message that moves is a change of
the documented surface.  ORDER pins what a call with two faults reports -- the one order include/sift_hip.h states --
and that a single-pair entry point and its one-pair batch refuse by the same rule.
"""
import ctypes
import math

import numpy as np
import pytest

INVALID = -1  # SIFT_HIP_ERR_INVALID
MODELS = ("fundamental", "homography")
# (operation, model, batched, form)
ENTRIES = [(op, m, b, form) for op in ("verify", "refine") for m in MODELS for b in (False, True)
           for form in ("device", "host")] + [("score", m, False, "device") for m in MODELS]
GOOD = dict(matches=True, qxy=True, txy=True, nq=4, nt=4, cap=4, qs=3, ts=3, P=2, pairs=True, params=True, result=True,
            M=True, counts=True, mask=True, out="apart", K=16, max_error=1.5, rounds=1)
# One broken rule each, of those judged without the handle; `on` says which entry points have the rule.  A fault of one
# pair (cap, nq, nt, qxy, txy) is the last pair's in a batch.
FAULTS = {
    "null_pairs": (dict(pairs=False), lambda e: e[2]),
    "null_params": (dict(params=False), lambda e: e[0] == "verify"),
    "null_result": (dict(result=False), lambda e: e[0] != "score"),
    "null_model": (dict(M=False), lambda e: e[0] == "score"),
    "null_counts": (dict(counts=False), lambda e: e[0] == "score"),
    "P_0": (dict(P=0), lambda e: e[2]),
    "P_65": (dict(P=65), lambda e: e[2]),
    "qstride_1": (dict(qs=1), lambda e: True),
    "tstride_1": (dict(ts=1), lambda e: True),
    "cap_neg": (dict(cap=-1), lambda e: True),
    "cap_65537": (dict(cap=65537), lambda e: True),
    "nq_neg": (dict(nq=-1), lambda e: True),
    "nt_neg": (dict(nt=-1), lambda e: True),
    "null_qxy": (dict(qxy=False), lambda e: True),
    "null_txy": (dict(txy=False), lambda e: True),
    "null_matches": (dict(matches=False), lambda e: True),
    "max_error_0": (dict(max_error=0.0), lambda e: True),
    "max_error_nan": (dict(max_error=math.nan), lambda e: True),
    "max_error_inf": (dict(max_error=math.inf), lambda e: True),
    "out_is_matches": (dict(out="same"), lambda e: e[0] != "score" and e[3] == "device"),
    "out_overlaps": (dict(out="overlap"), lambda e: e[0] != "score" and e[3] == "device"),
    "null_mask": (dict(mask=False), lambda e: e[0] == "refine"),
    "rounds_0": (dict(rounds=0), lambda e: e[0] == "refine"),
    "rounds_9": (dict(rounds=9), lambda e: e[0] == "refine"),
    "K_0": (dict(K=0), lambda e: e[0] != "refine"),
    "K_4097": (dict(K=4097), lambda e: e[0] != "refine"),
}
# The handle's limits on a valid call: the stand-in's (max_matches, max_hypotheses, max_pairs), of which exactly one is
# too small for the call (cap 4 or caps 4 + 4, K 16 -- a refine call needs 1 --, P 2).
LIMITS = {
    "over_max_hypotheses": (100, 0, 64),
    "over_max_pairs": (100, 16, 1),
    "over_max_matches": (3, 16, 64),
}


def entry_name(e):
    op, model, batched, form = e
    return f"sift_hip_{op}_{model}{'_batched' if batched else ''}_{form}"


class Calls:
    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)

    def stand_in(self, limits):
        """A block in place of a verifier whose first ints are the handle's device, max_matches, max_hypotheses and
        max_pairs; every pointer in it is null, so it serves only calls that are refused."""
        self.fake[:] = 0
        self.fake.view(np.int32)[1:4] = limits
        return self.fake.ctypes.data

    def run(self, e, v, **faults):
        a = dict(GOOD, **faults)
        op, model, batched, form = e
        fn = getattr(self.L, entry_name(e))
        p = self.buf.ctypes.data
        P = a["P"]
        rows = (a["cap"] if 0 < a["cap"] <= 65536 else 0) + (4 * (P - 1) if batched and 0 < P <= 64 else 0)
        m, q, t = (p if a["matches"] else None), (p + 512 if a["qxy"] else None), (p + 512 if a["txy"] else None)
        res, mask = (p + 640 if a["result"] else None), (p + 700 if a["mask"] else None)
        out = {"apart": p + 768, "same": p, "overlap": p + 16 * max(rows - 1, 0)}[a["out"]]
        prm = self.sift._VerifyParams(a["K"], 0, a["max_error"])
        pp = ctypes.byref(prm) if a["params"] else None
        if batched:
            n = max(min(P, 64), 1)
            table = (self.sift._VerifyPair * n)(*([self.sift._VerifyPair(p + 512, p + 512, 4, 4, 4)] * (n - 1)
                                                  + [self.sift._VerifyPair(q, t, a["nq"], a["nt"], a["cap"])]))
            head = [v, m, None, P, table if a["pairs"] else None, a["qs"], a["ts"]]
        else:
            head = [v, m, None, a["cap"], q, a["qs"], a["nq"], t, a["ts"], a["nt"]]
        if op == "verify":
            tail = [pp, res, out, None, None, None] if form == "device" else [pp, res, p + 768, p + 900]
        elif op == "refine":
            tail = [a["max_error"], a["rounds"], res, mask] + ([out, None, None, None] if form == "device"
                                                               else [p + 768, None, None])
        else:
            tail = [p + 640 if a["M"] else None, a["K"], a["max_error"], p + 700 if a["counts"] else None, None]
        args = [ctypes.cast(ctypes.c_void_p(x), ty) if isinstance(x, int) and hasattr(ty, "contents") else x
                for x, ty in zip(head + tail, fn.argtypes)]
        assert len(args) == len(fn.argtypes)
        before = self.fake.copy()
        rc, msg = fn(*args), self.L.sift_hip_last_error().decode()
        assert not self.buf.any() and np.array_equal(self.fake, before), "a refused call wrote host memory"
        return rc, msg


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


def table(calls):
    """Every (entry point, handle, fault) of the pinned table -> (status, message)."""
    got = {}
    for e in ENTRIES:
        name = entry_name(e)
        for handle in ("null", "zeroed"):
            for fault, (kw, on) in FAULTS.items():
                if on(e):
                    v = None if handle == "null" else calls.stand_in((0, 0, 0))
                    got[f"{name} {handle} {fault}"] = calls.run(e, v, **kw)
        for limit, limits in LIMITS.items():
            if limit == "over_max_pairs" and not e[2]:
                continue
            got[f"{name} limit {limit}"] = calls.run(e, calls.stand_in(limits))
    return got


# "<handle> <fault>" -> {message: which entry points report it}; every status is SIFT_HIP_ERR_INVALID.
SELECT = {
    "*": lambda e: True,
    "single": lambda e: not e[2],
    "batched": lambda e: e[2],
    "refine single": lambda e: e[0] == "refine" and not e[2],
    "not refine single": lambda e: not (e[0] == "refine" and not e[2]),
    "fundamental": lambda e: e[1] == "fundamental",
    "homography": lambda e: e[1] == "homography",
}
NULL = {"null verifier": "*"}
PER_PAIR = lambda msg: {msg: "single", msg + " (pair 1)": "batched"}  # noqa: E731
EXPECTED = {
    **{f"null {fault}": NULL for fault in FAULTS},
    "zeroed null_pairs": {"verify: null pairs": "*"},
    "zeroed null_params": {"verify: null params or result": "*"},
    "zeroed null_result": {"verify: null params or result": "not refine single", "refine: null result": "refine single"},
    "zeroed null_model": {"verify: null F or counts": "fundamental", "verify: null H or counts": "homography"},
    "zeroed null_counts": {"verify: null F or counts": "fundamental", "verify: null H or counts": "homography"},
    "zeroed P_0": {"verify: pairs outside 1..64": "*"},
    "zeroed P_65": {"verify: pairs outside 1..64": "*"},
    "zeroed qstride_1": {"verify: a position stride below 2 floats": "*"},
    "zeroed tstride_1": {"verify: a position stride below 2 floats": "*"},
    "zeroed cap_neg": PER_PAIR("verify: cap must lie in 0..65536"),
    "zeroed cap_65537": PER_PAIR("verify: cap must lie in 0..65536"),
    "zeroed nq_neg": PER_PAIR("verify: a negative position row count"),
    "zeroed nt_neg": PER_PAIR("verify: a negative position row count"),
    "zeroed null_qxy": PER_PAIR("verify: null position pointer"),
    "zeroed null_txy": PER_PAIR("verify: null position pointer"),
    "zeroed null_matches": {"verify: null matches": "*"},
    "zeroed max_error_0": {"verify: max_error must be > 0 and finite": "*"},
    "zeroed max_error_nan": {"verify: max_error must be > 0 and finite": "*"},
    "zeroed max_error_inf": {"verify: max_error must be > 0 and finite": "*"},
    "zeroed out_is_matches": {"verify: out aliases matches": "*"},
    "zeroed out_overlaps": {"verify: out aliases matches": "*"},
    "zeroed null_mask": {"refine: null mask (the mask is the fit set)": "*"},
    "zeroed rounds_0": {"refine: rounds must lie in 1..8": "*"},
    "zeroed rounds_9": {"refine: rounds must lie in 1..8": "*"},
    "zeroed K_0": {"verify: hypotheses outside 1..max_hypotheses": "*"},
    "zeroed K_4097": {"verify: hypotheses outside 1..max_hypotheses": "*"},
    "limit over_max_hypotheses": {"verify: hypotheses outside 1..max_hypotheses": "*"},
    "limit over_max_pairs": {"verify: more pairs than the verifier's max_pairs": "*"},
    "limit over_max_matches": {"verify: cap exceeds the verifier's max_matches": "single",
                               "verify: the caps' sum exceeds the verifier's max_matches": "batched"},
}


def test_refusals_are_the_pinned_ones(calls):
    got = table(calls)
    assert len(got) > 600 and {k.split(" ", 1)[1] for k in got} == set(EXPECTED)
    by_name = {entry_name(e): e for e in ENTRIES}
    for k, (rc, msg) in got.items():
        name, case = k.split(" ", 1)
        want = [m for m, who in EXPECTED[case].items() if SELECT[who](by_name[name])]
        assert len(want) == 1 and (rc, msg) == (INVALID, want[0]), k


# Two faults in one call: the rule reported is the first in the order of include/sift_hip.h, whatever the entry point.
# (the faults, on which operations and forms, the message of the single-pair call, of the one-pair batch)
PARAMS_OR_RESULT = "verify: null params or result"
STRIDE = "verify: a position stride below 2 floats"
CAP = "verify: cap must lie in 0..65536"
POSITION = "verify: null position pointer"
MAX_ERROR = "verify: max_error must be > 0 and finite"
ALIAS = "verify: out aliases matches"
ORDER = [
    (("null_params", "qstride_1"), ("verify",), ("device", "host"), PARAMS_OR_RESULT, PARAMS_OR_RESULT),
    (("null_result", "cap_65537"), ("verify",), ("device", "host"), PARAMS_OR_RESULT, PARAMS_OR_RESULT),
    (("null_result", "cap_65537"), ("refine",), ("device", "host"), "refine: null result", PARAMS_OR_RESULT),
    (("null_model", "cap_neg"), ("score",), ("device",), "verify: null {M} or counts", None),
    (("tstride_1", "cap_neg"), ("verify", "refine", "score"), ("device", "host"), STRIDE, STRIDE),
    (("cap_65537", "nq_neg"), ("verify", "refine", "score"), ("device", "host"), CAP, CAP + " (pair 0)"),
    (("nt_neg", "null_qxy"), ("verify", "refine", "score"), ("device", "host"),
     "verify: a negative position row count", "verify: a negative position row count (pair 0)"),
    (("null_txy", "null_matches"), ("verify", "refine", "score"), ("device", "host"), POSITION, POSITION + " (pair 0)"),
    (("null_matches", "max_error_nan"), ("verify", "refine", "score"), ("device", "host"), "verify: null matches",
     "verify: null matches"),
    (("max_error_0", "out_is_matches"), ("verify", "refine"), ("device",), MAX_ERROR, MAX_ERROR),
    (("max_error_0", "rounds_9"), ("refine",), ("device", "host"), MAX_ERROR, MAX_ERROR),
    (("out_overlaps", "null_mask"), ("refine",), ("device",), ALIAS, ALIAS),
    (("null_mask", "rounds_0"), ("refine",), ("device", "host"), "refine: null mask (the mask is the fit set)",
     "refine: null mask (the mask is the fit set)"),
    (("out_is_matches", "K_4097"), ("verify",), ("device",), ALIAS, ALIAS),
]


def rule(msg):
    """The rule behind a message: a batch names the pair, and words a missing result record as the verify calls do."""
    return msg.split(" (pair ")[0].replace("refine: null result", PARAMS_OR_RESULT)


@pytest.mark.parametrize("case", ORDER, ids=lambda c: "+".join(c[0]) + "-" + "_".join(c[1]))
def test_two_faults_report_the_first_rule_of_the_shared_order(calls, case):
    faults, ops, forms, single, batch = case
    kw = {k: v for f in faults for k, v in FAULTS[f][0].items()}
    for op in ops:
        for model in MODELS:
            for form in forms:
                if op == "score" and form == "host":
                    continue
                rc, msg = calls.run((op, model, False, form), calls.stand_in((0, 0, 0)), **kw)
                assert (rc, msg) == (INVALID, single.format(M="H" if model == "homography" else "F")), (op, model, form)
                if op == "score":
                    continue
                rc1, msg1 = calls.run((op, model, True, form), calls.stand_in((0, 0, 0)), P=1, **kw)
                assert (rc1, msg1) == (INVALID, batch), (op, model, form)
                assert rule(msg1) == rule(msg)
