"""Essential-matrix verification (sift_hip_verifier_reserve_essential, sift_hip_verify_essential_*): what runs
without a GPU, after tests/test_affine_abi.py.

* The entry points are exported with the signatures include/sift_hip.h documents; the record is the fundamental
  matrix's 52-byte sift_hip_verify_result; the ABI version is still 1.
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, and a verifier without the
  essential scratch is SIFT_HIP_ERR_STATE, with nothing launched: the calls run on host memory that is never read or
  written and on a verifier that is null, or a zeroed block standing in for one (`limits` gives it a max_matches and a
  max_pairs so that a call in order reaches the reservation rule, still before any device call).
* The hypotheses getter refuses a verifier no essential call has run on.
* The Python and C++ surfaces exist.
(`hypotheses` above a reservation needs a reservation, so a GPU: tests/test_gpu_essential.py.)
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
INVALID, STATE = -1, -3  # SIFT_HIP_ERR_INVALID, SIFT_HIP_ERR_STATE

ARGS = {"sift_hip_verifier_reserve_essential": 2, "sift_hip_verify_essential_device": 18,
        "sift_hip_verify_essential_host": 16, "sift_hip_verify_essential_batched_device": 15,
        "sift_hip_verify_essential_batched_host": 13, "sift_hip_verify_essential_hypotheses_host": 5}
SIGNATURES = """
#include "sift_hip.h"
#define ONE const int*, int, const float*, int, int, const float*, int, int
#define MANY const int*, int, const sift_hip_verify_pair*, int, int
#define CAMS const sift_hip_camera*, const sift_hip_camera*
int (*r)(sift_hip_verifier_t, int) = sift_hip_verifier_reserve_essential;
int (*a)(sift_hip_verifier_t, const sift_hip_dmatch*, ONE, CAMS, const sift_hip_verify_params*, sift_hip_verify_result*,
         sift_hip_dmatch*, int*, uint8_t*, void*) = sift_hip_verify_essential_device;
int (*b)(sift_hip_verifier_t, const sift_hip_dmatch*, ONE, CAMS, const sift_hip_verify_params*, sift_hip_verify_result*,
         sift_hip_dmatch*, uint8_t*) = sift_hip_verify_essential_host;
int (*c)(sift_hip_verifier_t, const sift_hip_dmatch*, MANY, CAMS, const sift_hip_verify_params*, sift_hip_verify_result*,
         sift_hip_dmatch*, int*, uint8_t*, void*) = sift_hip_verify_essential_batched_device;
int (*d)(sift_hip_verifier_t, const sift_hip_dmatch*, MANY, CAMS, const sift_hip_verify_params*, sift_hip_verify_result*,
         sift_hip_dmatch*, uint8_t*) = sift_hip_verify_essential_batched_host;
int (*e)(sift_hip_verifier_t, int*, float*, int*, int) = sift_hip_verify_essential_hypotheses_host;
int layout[] = {sizeof(sift_hip_verify_result), sizeof(sift_hip_camera), SIFT_HIP_ABI_VERSION};
"""


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name, n in ARGS.items():
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == n, name
    assert "abi=1" in sift.version()
    sig = tmp_path / "signatures.c"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    assert ctypes.sizeof(sift._VerifyResult) == 52 and sift.VERIFY_RESULT_DTYPE.itemsize == 52


def test_surfaces_exist(sift):
    from sift_amd import cv

    V = sift.Verifier
    for name, twin in (("verify_essential_device", "verify_device"), ("verify_essential_host", "verify_host"),
                       ("verify_essential_batched_device", "verify_batched_device"),
                       ("verify_essential_batched_host", "verify_batched_host")):
        got = list(inspect.signature(getattr(V, name)).parameters)
        want = list(inspect.signature(getattr(V, twin)).parameters)
        cams = ["cam_q", "cam_t"] if "batched" not in name else ["cams_q", "cams_t"]
        at = want.index("nt") + 1 if "batched" not in name else want.index("pairs") + 1
        assert got == want[:at] + cams + want[at:], name  # the fundamental form with the cameras behind the positions
    assert "essential_samples" in inspect.signature(V.__init__).parameters
    assert inspect.signature(V.__init__).parameters["essential_samples"].default == 0
    assert callable(V.reserve_essential) and callable(V.essential_hypotheses)
    assert list(inspect.signature(cv.essential_samples).parameters) == ["n", "K", "seed"]
    assert list(inspect.signature(cv.essential_from_5).parameters)[:4] == ["q_xy5", "t_xy5", "cam_q", "cam_t"]
    assert list(inspect.signature(cv.ransac_essential).parameters) == ["matches", "q_xy", "t_xy", "cam_q", "cam_t",
                                                                       "max_error", "K", "seed"]
    assert list(inspect.signature(sift.verifyEssential).parameters)[:7] == ["matches", "des_xy", "src_xy", "n_des", "n_src",
                                                                            "cam_q", "cam_t"]
    assert "refit" in inspect.signature(sift.verifyEssential).parameters
    assert list(inspect.signature(sift.verifyEssentialBatched).parameters)[:4] == ["matches_per_pair", "xy_per_pair",
                                                                                   "cams_q", "cams_t"]
    assert (cv.ESSENTIAL_SLOTS, cv.ESSENTIAL_BISECTIONS, cv.ESSENTIAL_NEWTON) == (10, 48, 3)


GOOD_CAM = (700.0, 710.0, 320.0, 240.0)


class Calls:
    """The four verify entry points on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed 512-byte block in place of a verifier: limits 0, no reservation

    def verifier(self, v):
        """None, the zeroed block ("fake"), or the block with max_matches = 64 and max_pairs = 2 ("limits": the four
        leading ints of the handle are device, max_matches, max_hypotheses, max_pairs)."""
        head = np.int32([0, 64, 0, 2] if v == "limits" else [0, 0, 0, 0])
        self.fake[:2] = head.view(np.int64)
        return (None if v is None else ctypes.c_void_p(self.fake.ctypes.data)), head.tobytes()

    def run(self, v="limits", matches=True, cap=4, qxy=True, qs=3, nq=4, txy=True, ts=3, nt=4, cam_q=GOOD_CAM,
            cam_t=GOOD_CAM, params="good", result=True, out="apart", K=16, max_error=1.5):
        """(rc, message) of verify_essential_device, _host, _batched_device and _batched_host."""
        L, p, S = self.L, self.buf.ctypes.data, self.sift
        vp, head = self.verifier(v)
        prm = S._VerifyParams(K, 0, max_error)
        pp = ctypes.byref(prm) if params == "good" else None
        res = S._VerifyResult()
        cq = (S._Camera * 1)(S._Camera(*cam_q)) if cam_q else None
        ct = (S._Camera * 1)(S._Camera(*cam_t)) if cam_t else None
        mp, qp, tp = (p if matches else None), (p + 512 if qxy else None), (p + 512 if txy else None)
        op = {"apart": p + 768, "same": p, None: None}[out]
        rp = p + 640 if result else None
        lst = (mp, None, cap, qp, qs, nq, tp, ts, nt)
        table = (S._VerifyPair * 1)(S._VerifyPair(qp, tp, nq, nt, cap))
        many = (mp, None, 1, table, qs, ts)
        got = [
            (L.sift_hip_verify_essential_device(vp, *lst, cq, ct, pp, rp, op, None, None, None), L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_essential_host(vp, *lst, cq, ct, pp, ctypes.byref(res) if result else None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_essential_batched_device(vp, *many, cq, ct, pp, rp, op, None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_essential_batched_host(vp, *many, cq, ct, pp, ctypes.byref(res) if result else None, None, None),
             L.sift_hip_last_error().decode()),
        ]
        assert not self.buf.any() and self.fake.tobytes()[:16] == head and not self.fake[2:].any()
        assert bytes(res) == bytes(52)
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


def test_a_verifier_that_has_not_reserved_is_the_state_error(calls):
    for rc, msg in calls.run():  # every argument in order
        assert rc == STATE and "essential scratch" in msg, msg
    for rc, msg in calls.run(cap=0, matches=False, qxy=False, txy=False, out=None):  # the empty list reaches it too
        assert rc == STATE and "essential scratch" in msg, msg


def test_null_verifier_params_or_result(calls):
    for rc, msg in calls.run(v=None):
        assert rc == INVALID and "verifier" in msg, msg
    for rc, msg in calls.run(params=None):
        assert rc == INVALID and "params" in msg, msg
    for rc, msg in calls.run(result=False):
        assert rc == INVALID and "result" in msg, msg


@pytest.mark.parametrize("side", ["cam_q", "cam_t"])
def test_bad_cameras_are_refused(calls, side):
    for rc, msg in calls.run(**{side: None}):
        assert rc == INVALID and "camera" in msg, msg
    for bad in ((0.0, 700, 320, 240), (700, -1.0, 320, 240), (math.nan, 700, 320, 240), (700, math.inf, 320, 240)):
        for rc, msg in calls.run(**{side: bad}):
            assert rc == INVALID and "fx and fy" in msg, msg
    for bad in ((700, 700, math.nan, 240), (700, 700, 320, -math.inf)):
        for rc, msg in calls.run(**{side: bad}):
            assert rc == INVALID and "cx and cy" in msg, msg


@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, cap):
    for rc, msg in calls.run(cap=cap):
        assert rc == INVALID and "cap" in msg, msg


def test_limits_of_the_verifier(calls):
    for rc, msg in calls.run(cap=65, out=None):  # the stand-in's max_matches is 64
        assert rc == INVALID and "max_matches" in msg, msg
    for rc, msg in calls.run(v="fake"):  # max_pairs 0
        assert rc == INVALID and "max_pairs" in msg, msg


@pytest.mark.parametrize("K", [0, -1, 4097])
def test_bad_hypotheses_is_refused(calls, K):
    for rc, msg in calls.run(K=K):
        assert rc == INVALID and "hypotheses" in msg, msg


def test_hypotheses_are_not_bound_by_max_hypotheses(calls):
    for rc, msg in calls.run(K=4096):  # the stand-in's max_hypotheses is 0: the reservation is the bound
        assert rc == STATE and "essential scratch" in msg, msg


@pytest.mark.parametrize("max_error", [0.0, -0.0, -1.5, float("nan"), math.inf, -math.inf])
def test_bad_max_error_is_refused(calls, max_error):
    for rc, msg in calls.run(max_error=max_error):
        assert rc == INVALID and "max_error" in msg, msg


@pytest.mark.parametrize("strides", [(1, 3), (3, 1), (0, 2), (-3, 3)])
def test_bad_stride_is_refused(calls, strides):
    for rc, msg in calls.run(qs=strides[0], ts=strides[1]):
        assert rc == INVALID and "stride" in msg, msg


def test_null_pointers_with_a_non_empty_list_are_refused(calls):
    for rc, msg in calls.run(matches=False):
        assert rc == INVALID and "matches" in msg, msg
    for kw in (dict(qxy=False), dict(txy=False)):
        for rc, msg in calls.run(**kw):
            assert rc == INVALID and "position" in msg, msg
    for kw in (dict(nq=-1), dict(nt=-1)):
        for rc, msg in calls.run(**kw):
            assert rc == INVALID and "row count" in msg, msg
    got = calls.run(out="same")
    for rc, msg in (got[0], got[2]):
        assert rc == INVALID and "alias" in msg, msg


def test_reserve_refusals(calls):
    L = calls.L
    fake, _ = calls.verifier("limits")
    assert L.sift_hip_verifier_reserve_essential(None, 16) == INVALID and b"verifier" in L.sift_hip_last_error()
    for n in (0, -1, 4097):
        assert L.sift_hip_verifier_reserve_essential(fake, n) == INVALID and b"max_samples" in L.sift_hip_last_error()


def test_getters_refuse_each_other(calls):
    """The essential getter refuses a verifier without an essential call; the other getters' refusals after an essential
    call need one to have run (tests/test_gpu_essential.py)."""
    L = calls.L
    fake, _ = calls.verifier("limits")
    out = np.zeros(64, np.int32)
    fn = L.sift_hip_verify_essential_hypotheses_host
    assert fn(None, None, None, None, 4) == INVALID and b"verifier" in L.sift_hip_last_error()
    assert fn(fake, None, None, None, -1) == INVALID and b"cap" in L.sift_hip_last_error()
    assert fn(fake, out.ctypes.data, None, None, 4) == STATE and L.sift_hip_last_error()
    assert not out.any()
