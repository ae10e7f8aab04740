"""Inputs shared by the batched verification tests (tests/test_verify_batched_cases.py,
tests/test_gpu_verify_batched.py, tests/test_gpu_verify_batched_cxx.py), on top of tests/verify_cases.py and
tests/homography_cases.py, which are imported and not edited.

A batch is a list of pairs; pair p is a buffer of cap records (its rows of the call's match array), the number of
records that count when the call takes its counts from the device, and its two position arrays.  The rule of a batched
call: pair p's outputs are sift_amd.cv.ransac_fundamental / ransac_homography of the records that count, with the call's
K and max_error and the seed (seed + p) mod 2^32.

MIXED, K = 256: caps that are no multiples of 64 -- a list below the sample size, (120, 80), an empty pair, the CAPPED
    list (129 counted records at the head of a buffer of 200 whose tail must not count: its count comes from the device
    counter), (300, 300), (24, 9), and make(1800, 313): 2113 records, past the score kernel's 2048-match LDS tile and
    the select kernel's 1024-row chunks.  The short list comes first so that (120, 80) and (300, 300) sit at p > 0,
    where ignoring p in the seed shows; the seed is 2^32 - 3, so seed + p wraps from pair 3 on.
LARGE64, K = 64: (24, 9) and the 2113-record pair again, at the K tests/homography_cases.LARGE uses.
FULL, K = 64: 64 pairs make(24, 9, seed=p), the most a call takes.
SPILL: caps (65536, 70000) on a verifier of max_matches = 140000 -- refusal cases only, never run.
"""
import functools

import numpy as np

import homography_cases as hc
import verify_cases as vc

MAX_ERROR = 1.5
MODELS = ("fundamental", "homography")
CASES = {"fundamental": vc, "homography": hc}
SAMPLE = {"fundamental": 8, "homography": 4}
SHORT = {"fundamental": (7, 0), "homography": (3, 0)}
LARGE = (1800, 313)
BATCHES = {"MIXED": (256, 2 ** 32 - 3), "LARGE64": (64, 11), "FULL": (64, 7)}
SPILL = dict(caps=(65536, 70000), max_matches=140000)
U32 = 2 ** 32


def rule(model):
    from sift_amd import cv

    return cv.ransac_fundamental if model == "fundamental" else cv.ransac_homography


def _empty(model):
    from sift_amd import DMATCH_DTYPE

    # one position row per side for the numpy rule (it takes no empty array); the device gets null pointers and 0 rows
    return np.zeros(0, DMATCH_DTYPE), np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32)


@functools.lru_cache(maxsize=None)
def pairs(model, batch):
    """The batch's pairs: dicts of buf (cap records), count (the records that count under a device counter), q_xy,
    t_xy and shape, a label.  Read-only."""
    mod = CASES[model]

    def whole(shape, seed=None):
        m, q_xy, t_xy, _ = mod.case(*shape) if seed is None else mod.make(*shape, seed=seed)
        return dict(buf=m, count=len(m), q_xy=q_xy, t_xy=t_xy, shape=shape)

    if batch == "MIXED":
        e = _empty(model)
        c = mod.case(*mod.CAPPED[:2])
        out = [whole(SHORT[model]), whole((120, 80)), dict(buf=e[0], count=0, q_xy=e[1], t_xy=e[2], shape="empty"),
               dict(buf=mod.capped(), count=len(c[0]), q_xy=c[1], t_xy=c[2], shape="capped"), whole((300, 300)),
               whole((24, 9)), whole(LARGE)]
    elif batch == "LARGE64":
        out = [whole((24, 9)), whole(LARGE)]
    elif batch == "FULL":
        out = [whole((24, 9), seed=p) for p in range(64)]
    else:
        raise KeyError(batch)
    for p in out:
        for a in p.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def caps(model, batch):
    return [len(p["buf"]) for p in pairs(model, batch)]


def row0(model, batch):
    return np.concatenate([[0], np.cumsum(caps(model, batch))]).astype(int)


def matches(model, batch):
    """Every pair's buffer, pair p's rows at row0[p]: the call's match array."""
    return np.concatenate([p["buf"] for p in pairs(model, batch)])


def counts(model, batch):
    """The device counters: the records of each pair that count."""
    return np.int32([p["count"] for p in pairs(model, batch)])


@functools.lru_cache(maxsize=None)
def reference(model, batch, p, counted=True, seed_offset=True):
    """The rule for pair p: of its counted records (counted: the device counter's number, else all cap rows), with the
    seed (seed + p) mod 2^32 (seed_offset False: the call's own seed, what a kernel that ignores p would draw with).
    Computed once and shared; read-only."""
    K, seed = BATCHES[batch]
    pr = pairs(model, batch)[p]
    n = pr["count"] if counted else len(pr["buf"])
    r = rule(model)(pr["buf"][:n], pr["q_xy"], pr["t_xy"], MAX_ERROR, K, (seed + p) % U32 if seed_offset else seed)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def model_of(model, ref):
    return ref["F" if model == "fundamental" else "H"]
