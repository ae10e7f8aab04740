"""The refit entry points (sift_hip_refine_*): what runs without a GPU, after tests/test_verify_batched_abi.py.

* The eight entry points are exported with the signatures include/sift_hip.h documents; the ABI version stays 1.
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, and nothing is launched: the calls
  run on host memory that is never read or written and on a verifier that is null, or a zeroed block standing in for
  one (limits 0: whatever reaches the limit rules is refused there, still before any device call).
* The Python surface exists, and the numpy rule refuses what the calls refuse.
"""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
INVALID = -1  # SIFT_HIP_ERR_INVALID
MODELS = ("fundamental", "homography")
NAMES = tuple(f"sift_hip_refine_{m}{b}_{w}" for m in MODELS for b in ("", "_batched") for w in ("device", "host"))
SIGNATURES = "\n#include \"sift_hip.h\"\n" + "\n".join(f"""
int (*a_{m})(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
             float, int, {r}*, uint8_t*, sift_hip_dmatch*, int*, int*, void*) = sift_hip_refine_{m}_device;
int (*b_{m})(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
             float, int, {r}*, uint8_t*, sift_hip_dmatch*, int*, int*) = sift_hip_refine_{m}_host;
int (*c_{m})(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int, float,
             int, {r}*, uint8_t*, sift_hip_dmatch*, int*, int*, void*) = sift_hip_refine_{m}_batched_device;
int (*d_{m})(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int, float,
             int, {r}*, uint8_t*, sift_hip_dmatch*, int*, int*) = sift_hip_refine_{m}_batched_host;
""" for m, r in (("fundamental", "sift_hip_verify_result"), ("homography", "sift_hip_homography_result"))) + """
int abi[SIFT_HIP_ABI_VERSION == 1 ? 1 : -1];
int params[sizeof(sift_hip_verify_params) == 12 ? 1 : -1];
"""


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
        want = {("device", False): 18, ("host", False): 17, ("device", True): 15, ("host", True): 14}
        assert len(getattr(L, name).argtypes) == want[(name.rsplit("_", 1)[1], "batched" in name)], name
    assert "abi=1" in sift.version()
    sig = tmp_path / "signatures.c"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)


def test_surfaces_exist(sift):
    from sift_amd import cv

    for name in ("refine_device", "refine_homography_device", "refine_host", "refine_homography_host"):
        sig = list(inspect.signature(getattr(sift.Verifier, name)).parameters)
        assert sig[:8] == ["self", "matches_ptr", "count_ptr", "cap", "q_xy_ptr", "nq", "t_xy_ptr", "nt"], sig
        assert inspect.signature(getattr(sift.Verifier, name)).parameters["rounds"].default == 1
    for name in ("refine_batched_device", "refine_homography_batched_device", "refine_batched_host",
                 "refine_homography_batched_host"):
        sig = list(inspect.signature(getattr(sift.Verifier, name)).parameters)
        assert sig[:4] == ["self", "matches_ptr", "counts_ptr", "pairs"], sig
    for name in ("verifyFundamental", "verifyHomography", "verifyFundamentalBatched", "verifyHomographyBatched"):
        assert inspect.signature(getattr(sift, name)).parameters["refit"].default == 0
    for name in ("refit_fundamental", "refit_homography"):
        assert list(inspect.signature(getattr(cv, name)).parameters) == ["pts_or_matches", "q_xy", "t_xy", "mask"]
    for name in ("refine_fundamental", "refine_homography"):
        assert list(inspect.signature(getattr(cv, name)).parameters) == ["matches", "q_xy", "t_xy", "result", "max_error",
                                                                         "rounds"]
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    for name in ("refineDevice", "refineHomographyDevice", "refineHost", "refineHomographyHost", "refineBatchedDevice",
                 "refineHomographyBatchedDevice", "refineBatchedHost", "refineHomographyBatchedHost"):
        assert f"sift_cuda::Verifier::{name}(sift_cuda::DMatch const*, int const*, " in out, name
    for name in ("verifyFundamental", "verifyHomography"):  # the existing one shots and their refit overloads
        assert out.count(f"sift_cuda::{name}(std::vector<sift_cuda::DMatch") == 2, name
    with pytest.raises(ValueError):
        cv.refit_fundamental(np.zeros((9, 3), np.float32))
    with pytest.raises(ValueError):
        cv.refit_homography(np.zeros((9, 4), np.float32), mask=np.ones(5, np.uint8))


class Calls:
    """The eight entry points, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed block in place of a verifier: limits 0

    def run(self, batched, v="fake", matches=True, cap=4, caps=(4, 3), P=2, pairs="good", qxy=True, txy=True, nq=4, nt=4,
            qs=3, ts=3, result=True, mask=True, out="apart", max_error=1.5, rounds=1):
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        mp, qp, tp = p if matches else None, p + 512 if qxy else None, p + 512 if txy else None
        rp, kp = p + 640 if result else None, p + 700 if mask else None
        rows = sum(c for c in caps if 0 < c <= 65536) if batched else cap
        op = {"apart": p + 768, "same": p, "overlap": p + 16 * max(rows - 1, 0), None: None}[out]
        got = []
        for name in MODELS:
            if batched:
                table = (self.sift._VerifyPair * max(len(caps), 1))(*[self.sift._VerifyPair(qp, tp, nq, nt, c) for c in caps])
                tab = table if pairs == "good" else None
                dev = getattr(L, f"sift_hip_refine_{name}_batched_device")
                host = getattr(L, f"sift_hip_refine_{name}_batched_host")
                got.append((dev(vp, mp, None, P, tab, qs, ts, max_error, rounds, rp, kp, op, None, None, None),
                            L.sift_hip_last_error().decode()))
                got.append((host(vp, mp, None, P, tab, qs, ts, max_error, rounds, rp, kp, None, None, None),
                            L.sift_hip_last_error().decode()))
            else:
                dev = getattr(L, f"sift_hip_refine_{name}_device")
                host = getattr(L, f"sift_hip_refine_{name}_host")
                got.append((dev(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, max_error, rounds, rp, kp, op, None, None, None),
                            L.sift_hip_last_error().decode()))
                got.append((host(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, max_error, rounds, rp, kp, None, None, None),
                            L.sift_hip_last_error().decode()))
        assert not self.buf.any() and not self.fake.any()
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


BOTH = pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])


@BOTH
def test_null_verifier_result_or_mask(calls, batched):
    for rc, msg in calls.run(batched, v=None):
        assert rc == INVALID and "verifier" in msg, msg
    for rc, msg in calls.run(batched, result=False):
        assert rc == INVALID and "result" in msg, msg
    for rc, msg in calls.run(batched, mask=False):
        assert rc == INVALID and "mask" in msg, msg
    # no row, no mask needed: such a call reaches the stand-in's limits
    for rc, msg in calls.run(batched, mask=False, matches=False, qxy=False, txy=False, cap=0, caps=(0, 0)):
        assert rc == INVALID and ("hypotheses" in msg or "max_" in msg), msg


@BOTH
@pytest.mark.parametrize("rounds", [0, -1, 9, 2 ** 31 - 1])
def test_bad_rounds_is_refused(calls, batched, rounds):
    for rc, msg in calls.run(batched, rounds=rounds):
        assert rc == INVALID and "rounds must lie in 1..8" in msg, msg


@BOTH
@pytest.mark.parametrize("max_error", [0.0, -0.0, -1.5, float("nan"), math.inf, -math.inf])
def test_bad_max_error_is_refused(calls, batched, max_error):
    for rc, msg in calls.run(batched, max_error=max_error):
        assert rc == INVALID and "max_error" in msg, msg


@BOTH
@pytest.mark.parametrize("strides", [(1, 3), (3, 1), (0, 2), (-3, 3)])
def test_bad_stride_is_refused(calls, batched, strides):
    for rc, msg in calls.run(batched, qs=strides[0], ts=strides[1]):
        assert rc == INVALID and "stride" in msg, msg


@BOTH
@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, batched, cap):
    for rc, msg in calls.run(batched, cap=cap, caps=(4, cap)):
        assert rc == INVALID and "cap" in msg, msg


@BOTH
def test_null_pointers_and_negative_row_counts_are_refused(calls, batched):
    for rc, msg in calls.run(batched, matches=False):
        assert rc == INVALID and "matches" in msg, msg
    for kw in (dict(qxy=False), dict(txy=False)):
        for rc, msg in calls.run(batched, **kw):
            assert rc == INVALID and "position" in msg, msg
    for kw in (dict(nq=-1), dict(nt=-1)):
        for rc, msg in calls.run(batched, **kw):
            assert rc == INVALID and "row count" in msg, msg


def test_batch_table_rules(calls):
    for rc, msg in calls.run(True, pairs=None):
        assert rc == INVALID and "pairs" in msg, msg
    for P in (0, -1, 65):
        for rc, msg in calls.run(True, P=P):
            assert rc == INVALID and "pairs outside" in msg, msg


@BOTH
@pytest.mark.parametrize("out", ["same", "overlap"])
def test_out_aliasing_matches_is_refused(calls, batched, out):
    got = calls.run(batched, out=out)
    for rc, msg in (got[0], got[2]):  # the device forms
        assert rc == INVALID and "alias" in msg, msg


@BOTH
def test_limits_of_the_handle_are_respected(calls, batched):
    """Good arguments reach the stand-in's limits (all 0) and are refused there."""
    for rc, msg in calls.run(batched):
        assert rc == INVALID and ("hypotheses" in msg or "max_" in msg), msg
