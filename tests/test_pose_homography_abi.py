"""The plane pose entry points (sift_hip_recover_pose_homography_*): what runs without a GPU, after
tests/test_pose_abi.py.

* The four entry points are exported with the signatures include/sift_hip.h documents, and the four pose entry points
  beside them keep theirs; the ABI version stays 1; the 96-byte record and the 64-byte candidate have their documented
  layouts, in C and in the Python dtypes.
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, in the documented order, and
  nothing is launched: the calls run on host memory that is never read or written and on a verifier that is null, or a
  zeroed block standing in for one.
* The Python and C++ surfaces exist, and the numpy rule refuses what the calls refuse.
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
NAMES = tuple(f"sift_hip_recover_pose{m}{b}_{w}" for m in ("", "_homography") for b in ("", "_batched")
              for w in ("device", "host"))
SIGNATURES = """
#include <stddef.h>
#include "sift_hip.h"
int (*a)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_homography_result*, const uint8_t*, const sift_hip_camera*, const sift_hip_camera*,
         const sift_hip_pose_params*, sift_hip_plane_pose_result*, uint8_t*, float*, sift_hip_dmatch*, int*,
         sift_hip_plane_candidate*, void*) = sift_hip_recover_pose_homography_device;
int (*b)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_homography_result*, const uint8_t*, const sift_hip_camera*, const sift_hip_camera*,
         const sift_hip_pose_params*, sift_hip_plane_pose_result*, uint8_t*, float*, sift_hip_dmatch*, int*,
         sift_hip_plane_candidate*) = sift_hip_recover_pose_homography_host;
int (*c)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_homography_result*, const uint8_t*, const sift_hip_camera*, const sift_hip_camera*,
         const sift_hip_pose_params*, sift_hip_plane_pose_result*, uint8_t*, float*, sift_hip_dmatch*, int*,
         sift_hip_plane_candidate*, void*) = sift_hip_recover_pose_homography_batched_device;
int (*d)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_homography_result*, const uint8_t*, const sift_hip_camera*, const sift_hip_camera*,
         const sift_hip_pose_params*, sift_hip_plane_pose_result*, uint8_t*, float*, sift_hip_dmatch*, int*,
         sift_hip_plane_candidate*) = sift_hip_recover_pose_homography_batched_host;
int (*e)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_verify_result*, const uint8_t*, const sift_hip_camera*, const sift_hip_camera*,
         const sift_hip_pose_params*, sift_hip_pose_result*, uint8_t*, float*, sift_hip_dmatch*, int*, void*) =
    sift_hip_recover_pose_device;
int abi[SIFT_HIP_ABI_VERSION == 1 ? 1 : -1];
int plane[sizeof(sift_hip_plane_pose_result) == 96 ? 1 : -1];
int lead[sizeof(sift_hip_pose_result) == 80 && offsetof(sift_hip_plane_pose_result, normal) == 80 ? 1 : -1];
int same[offsetof(sift_hip_plane_pose_result, t) == offsetof(sift_hip_pose_result, t) &&
         offsetof(sift_hip_plane_pose_result, in_front) == offsetof(sift_hip_pose_result, in_front) &&
         offsetof(sift_hip_plane_pose_result, with_parallax) == offsetof(sift_hip_pose_result, with_parallax) &&
         offsetof(sift_hip_plane_pose_result, counts) == offsetof(sift_hip_pose_result, counts) &&
         offsetof(sift_hip_plane_pose_result, candidate) == offsetof(sift_hip_pose_result, candidate) &&
         offsetof(sift_hip_plane_pose_result, fit) == offsetof(sift_hip_pose_result, fit) ? 1 : -1];
int dist[offsetof(sift_hip_plane_pose_result, distance) == 92 ? 1 : -1];
int cand[sizeof(sift_hip_plane_candidate) == 64 && offsetof(sift_hip_plane_candidate, t) == 36 &&
         offsetof(sift_hip_plane_candidate, normal) == 48 && offsetof(sift_hip_plane_candidate, distance) == 60 ? 1 : -1];
int record[sizeof(sift_hip_homography_result) == 52 ? 1 : -1];
"""


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    assert len(NAMES) == 8
    for name in NAMES:
        assert name in exported, name
        want = {("device", False): 21, ("host", False): 20, ("device", True): 18, ("host", True): 17}
        extra = 1 if "homography" in name else 0  # the trailing candidates
        assert len(getattr(L, name).argtypes) == want[(name.rsplit("_", 1)[1], "batched" in name)] + extra, name
    assert "abi=1" in sift.version()
    sig = tmp_path / "signatures.c"
    sig.write_text(SIGNATURES)
    for compiler, std in (("gcc", "-std=c99"), ("g++", "-std=c++17")):
        subprocess.run([compiler, std, "-x", "c" if compiler == "gcc" else "c++", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        os.path.join(ROOT, "include"), str(sig)], check=True)


def test_records_match_the_dtypes(sift):
    pose, plane, cand = sift.POSE_RESULT_DTYPE, sift.PLANE_POSE_RESULT_DTYPE, sift.PLANE_CANDIDATE_DTYPE
    assert plane.itemsize == 96 and cand.itemsize == 64 and pose.itemsize == 80
    for k in pose.names:  # the first 80 bytes are a pose record as it lies
        assert plane.fields[k][:2] == pose.fields[k][:2], k
    assert plane.names == pose.names + ("normal", "distance")
    assert [plane.fields[k][1] for k in ("normal", "distance")] == [80, 92]
    assert plane.fields["normal"][0] == np.dtype(("<f4", (3,))) and plane.fields["distance"][0] == np.dtype("<f4")
    assert cand.names == ("R", "t", "normal", "distance")
    assert [cand.fields[k][1] for k in cand.names] == [0, 36, 48, 60]
    r = np.zeros(1, plane)
    r["candidate"], r["fit"], r["distance"] = -1, 7, 2.5
    assert r.view(np.uint8)[:80].view(pose)[0]["candidate"] == -1 and r.view(np.uint8)[:80].view(pose)[0]["fit"] == 7
    assert r.view(np.float32).reshape(-1)[23] == 2.5


def test_surfaces_exist(sift):
    from sift_amd import cv

    for name in ("recover_pose_homography_device", "recover_pose_homography_host"):
        sig = list(inspect.signature(getattr(sift.Verifier, name)).parameters)
        assert sig[:8] == ["self", "matches_ptr", "count_ptr", "cap", "q_xy_ptr", "nq", "t_xy_ptr", "nt"], sig
    for name in ("recover_pose_homography_batched_device", "recover_pose_homography_batched_host"):
        sig = list(inspect.signature(getattr(sift.Verifier, name)).parameters)
        assert sig[:4] == ["self", "matches_ptr", "counts_ptr", "pairs"], sig
    for name in ("recover_pose_homography_device", "recover_pose_homography_host", "recover_pose_homography_batched_device",
                 "recover_pose_homography_batched_host"):
        par = inspect.signature(getattr(sift.Verifier, name)).parameters
        assert par["max_depth"].default == 50.0 and par["max_cos_parallax"].default == 0.99998
    for name in ("recover_pose_homography_device", "recover_pose_homography_batched_device"):
        assert inspect.signature(getattr(sift.Verifier, name)).parameters["candidates_ptr"].default == 0
    assert list(inspect.signature(sift.recoverPoseHomography).parameters)[:9] == [
        "matches", "des_xy", "src_xy", "n_des", "n_src", "result", "mask", "cam_q", "cam_t"]
    assert callable(sift.recoverPoseHomographyBatched)
    assert list(inspect.signature(cv.recover_pose_homography).parameters) == list(inspect.signature(cv.recover_pose).parameters)
    assert list(inspect.signature(cv.calibrated_homography).parameters) == ["H", "cam_q", "cam_t"]
    assert inspect.signature(cv.decompose_homography).parameters["sweeps"].default == cv.REFIT_SWEEPS
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    for name in ("recoverPoseHomographyDevice", "recoverPoseHomographyHost", "recoverPoseHomographyBatchedDevice",
                 "recoverPoseHomographyBatchedHost"):
        assert f"sift_cuda::Verifier::{name}(sift_cuda::DMatch const*, int const*, " in out, name
    assert "sift_cuda::recoverPoseHomography(std::vector<sift_cuda::DMatch" in out


def test_the_mirror_refuses_what_the_calls_refuse(sift):
    from sift_amd import cv

    m = np.zeros(4, sift.DMATCH_DTYPE)
    xy = np.zeros((4, 2), np.float32)
    res = {"H": np.eye(3, dtype=np.float32), "hypothesis": 0}
    mask = np.ones(4, np.uint8)
    good = (500.0, 500.0, 320.0, 240.0)
    r = cv.recover_pose_homography(m, xy, xy, res, mask, good, good, math.inf, -1.0)  # the limits are allowed
    assert r["candidate"] == -1 and r["fit"] == 4 and r["candidates"].dtype == sift.PLANE_CANDIDATE_DTYPE  # H = I: w1 = w3
    cv.recover_pose_homography(m, xy, xy, res, mask, good, good, 50, 1.0)
    for cam in ((0, 500, 1, 1), (500, -1, 1, 1), (math.inf, 500, 1, 1), (500, math.nan, 1, 1), (500, 500, math.nan, 1),
                (500, 500, 1, math.inf), (500, 500, 1)):
        with pytest.raises(ValueError):
            cv.recover_pose_homography(m, xy, xy, res, mask, cam, good)
        with pytest.raises(ValueError):
            cv.recover_pose_homography(m, xy, xy, res, mask, good, cam)
        with pytest.raises(ValueError):
            cv.calibrated_homography(res["H"], good, cam)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="max_depth"):
            cv.recover_pose_homography(m, xy, xy, res, mask, good, good, bad)
    for bad in (1.5, -1.5, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_cos_parallax"):
            cv.recover_pose_homography(m, xy, xy, res, mask, good, good, 50, bad)
    with pytest.raises(ValueError, match="mask"):
        cv.recover_pose_homography(m, xy, xy, res, mask[:3], good, good)
    with pytest.raises(ValueError):
        cv.calibrated_homography(np.zeros(8, np.float32), good, good)


class Calls:
    """The four entry points, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(512, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed block in place of a verifier: limits 0

    def run(self, batched, v="fake", matches=True, cap=4, caps=(4, 3), P=2, pairs="good", qxy=True, txy=True, nq=4, nt=4,
            qs=3, ts=3, result=True, mask=True, out="apart", cam_q=(500, 500, 320, 240), cam_t=(400, 410, 300, 200),
            cams="good", params=True, pose=True, max_depth=50.0, max_cos=0.99998, bad_pair=None, candidates=True):
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        mp, qp, tp = p if matches else None, p + 512 if qxy else None, p + 512 if txy else None
        rp, kp, pp = p + 640 if result else None, p + 760 if mask else None, p + 1200 if pose else None
        cp = p + 1400 if candidates else None
        rows = sum(c for c in caps if 0 < c <= 65536) if batched else cap
        op = {"apart": p + 800, "same": p, "overlap": p + 16 * max(rows - 1, 0), None: None}[out]
        par = ctypes.byref(self.sift._PoseParams(max_depth, max_cos)) if params else None
        n = max(len(caps), 1) if batched else 1
        good = (500.0, 500.0, 320.0, 240.0)
        cq = (self.sift._Camera * n)(*[self.sift._Camera(*(good if bad_pair not in (None, i) else cam_q)) for i in range(n)])
        ct = (self.sift._Camera * n)(*[self.sift._Camera(*(good if bad_pair not in (None, i) else cam_t)) for i in range(n)])
        cqp, ctp = (cq, ct) if cams == "good" else ((None, ct) if cams == "no query" else (cq, None))
        got = []
        if batched:
            table = (self.sift._VerifyPair * max(len(caps), 1))(*[self.sift._VerifyPair(qp, tp, nq, nt, c) for c in caps])
            tab = table if pairs == "good" else None
            got.append((L.sift_hip_recover_pose_homography_batched_device(vp, mp, None, P, tab, qs, ts, rp, kp, cqp, ctp, par, pp,
                                                                          None, None, op, None, cp, None),
                        L.sift_hip_last_error().decode()))
            got.append((L.sift_hip_recover_pose_homography_batched_host(vp, mp, None, P, tab, qs, ts, rp, kp, cqp, ctp, par, pp,
                                                                        None, None, None, None, cp),
                        L.sift_hip_last_error().decode()))
        else:
            got.append((L.sift_hip_recover_pose_homography_device(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, rp, kp, cqp, ctp, par,
                                                                  pp, None, None, op, None, cp, None),
                        L.sift_hip_last_error().decode()))
            got.append((L.sift_hip_recover_pose_homography_host(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, rp, kp, cqp, ctp, par,
                                                                pp, None, None, None, None, cp),
                        L.sift_hip_last_error().decode()))
        assert not self.buf.any() and not self.fake.any()
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


BOTH = pytest.mark.parametrize("batched", [False, True], ids=["single", "batched"])
LIMITS = ("hypotheses", "max_")  # what the zeroed stand-in refuses: a call that gets there passed every other rule


def refused(got, *words):
    for rc, msg in got:
        assert rc == INVALID and any(w in msg for w in words), msg


@BOTH
def test_list_rules_come_first(calls, batched):
    refused(calls.run(batched, v=None), "verifier")
    refused(calls.run(batched, qs=1), "stride")
    refused(calls.run(batched, ts=0), "stride")
    for cap in (-1, 65537, 2 ** 31 - 1):
        refused(calls.run(batched, cap=cap, caps=(4, cap)), "cap")
    refused(calls.run(batched, nq=-1), "row count")
    refused(calls.run(batched, nt=-1), "row count")
    refused(calls.run(batched, qxy=False), "position")
    refused(calls.run(batched, txy=False), "position")
    refused(calls.run(batched, matches=False), "matches")
    # each of them wins over every pose rule
    bad = dict(cams="no query", cam_q=(0, 0, 0, 0), params=False, result=False, mask=False, max_depth=-1.0)
    refused(calls.run(batched, qs=1, **bad), "stride")
    refused(calls.run(batched, matches=False, **bad), "matches")


def test_batch_table_rules(calls):
    refused(calls.run(True, pairs=None), "pairs")
    for P in (0, -1, 65):
        refused(calls.run(True, P=P), "pairs outside")


@BOTH
def test_pose_rules_in_the_documented_order(calls, batched):
    inf, nan = math.inf, math.nan
    # each rule, with every later rule broken as well: the first one is reported
    later = [dict(params=False), dict(max_depth=-1.0), dict(max_cos=2.0), dict(mask=False), dict(out="same")]
    refused(calls.run(batched, cams="no query", cam_t=(0, 0, 0, 0), **{k: v for d in later for k, v in d.items()}), "camera pointer")
    refused(calls.run(batched, cams="no train"), "camera pointer")
    for cam in ((0, 500, 1, 1), (500, -0.0, 1, 1), (-3, 500, 1, 1), (inf, 500, 1, 1), (500, nan, 1, 1)):
        refused(calls.run(batched, cam_q=cam, cam_t=(500, 500, nan, 1), params=False, mask=False), "fx and fy")
        refused(calls.run(batched, cam_t=cam, result=False, max_depth=nan), "fx and fy")
    for cam in ((500, 500, nan, 1), (500, 500, 1, inf), (500, 500, -inf, 1)):
        refused(calls.run(batched, cam_q=cam, params=False, result=False), "cx and cy")
        refused(calls.run(batched, cam_t=cam, pose=False, max_cos=nan), "cx and cy")
    refused(calls.run(batched, params=False, mask=False), "params or result")
    refused(calls.run(batched, result=False, max_depth=0.0), "params or result")
    refused(calls.run(batched, pose=False, max_cos=2.0), "params or result")
    for bad in (0.0, -0.0, -1.0, nan, -inf):
        refused(calls.run(batched, max_depth=bad, max_cos=2.0, mask=False), "max_depth")
    for bad in (1.0000001, -1.5, nan, inf, -inf):
        refused(calls.run(batched, max_cos=bad, mask=False, out="same"), "max_cos_parallax")
    refused(calls.run(batched, mask=False, out="same"), "mask")
    got = calls.run(batched, out="same") + calls.run(batched, out="overlap")
    refused((got[0], got[2]), "alias")  # the device forms
    refused((got[1], got[3]), *LIMITS)  # the host forms take no device out


def test_a_batched_call_names_the_pair(calls):
    for rc, msg in calls.run(True, cam_t=(500, 0, 1, 1), bad_pair=1):
        assert rc == INVALID and "fx and fy" in msg and "(pair 1)" in msg, msg
    for rc, msg in calls.run(True, cam_q=(500, 500, math.nan, 1), bad_pair=0):
        assert rc == INVALID and "cx and cy" in msg and "(pair 0)" in msg, msg


@BOTH
def test_allowed_values_reach_the_limits_of_the_handle(calls, batched):
    """Good arguments -- +inf as max_depth, -1 and 1 as max_cos_parallax, no candidates, no mask where no row is read --
    reach the stand-in's limits (all 0) and are refused there."""
    refused(calls.run(batched), *LIMITS)
    refused(calls.run(batched, candidates=False), *LIMITS)
    refused(calls.run(batched, max_depth=math.inf, max_cos=-1.0), *LIMITS)
    refused(calls.run(batched, max_cos=1.0), *LIMITS)
    refused(calls.run(batched, mask=False, matches=False, qxy=False, txy=False, cap=0, caps=(0, 0)), *LIMITS)
