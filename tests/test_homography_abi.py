"""Homography verification and projection (sift_hip_verify_homography_*, sift_hip_score_homography_device,
sift_hip_project_homography_device): what runs without a GPU, after tests/test_verify_abi.py.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_homography_result has the
  layout of its ctypes mirror and its numpy dtype (52 bytes); the ABI version is still 1.
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, and nothing is launched: the
  calls run on host memory that is never read or written and on a verifier that is null, or a zeroed block standing
  in for one (limits 0: whatever reaches the limit rules is refused there, still before any device call).  The
  projection needs no handle; its refusals run on host memory too.
* Each hypotheses getter refuses a verifier no verify call of its model has run on.
* The Python and C++ surfaces exist.
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

NAMES = ("sift_hip_verify_homography_device", "sift_hip_verify_homography_host", "sift_hip_score_homography_device",
         "sift_hip_verify_homography_hypotheses_host", "sift_hip_project_homography_device")
SIGNATURES = """
#include "sift_hip.h"
int (*d)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_verify_params*, sift_hip_homography_result*, sift_hip_dmatch*, int*, uint8_t*, void*) =
    sift_hip_verify_homography_device;
int (*e)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_verify_params*, sift_hip_homography_result*, sift_hip_dmatch*, uint8_t*) =
    sift_hip_verify_homography_host;
int (*f)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const float*, int, float, int*, void*) = sift_hip_score_homography_device;
int (*g)(sift_hip_verifier_t, int*, float*, int*, int) = sift_hip_verify_homography_hypotheses_host;
int (*h)(const float*, const float*, int, int, float*, int, void*) = sift_hip_project_homography_device;
int state = SIFT_HIP_ERR_STATE, invalid = SIFT_HIP_ERR_INVALID, abi = SIFT_HIP_ABI_VERSION;
"""
RESULT_FIELDS = ("H", "inliers", "hypothesis", "matches", "valid_hypotheses")
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_homography_result), %s, SIFT_HIP_ERR_INVALID, SIFT_HIP_ERR_STATE, SIFT_HIP_ABI_VERSION};
int main(void) {
    for (unsigned i = 0; i < sizeof layout / sizeof *layout; i++) printf("%%d\\n", layout[i]);
    return 0;
}
""" % ", ".join(f"__builtin_offsetof(sift_hip_homography_result, {f})" for f in RESULT_FIELDS)


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
    assert len(L.sift_hip_verify_homography_device.argtypes) == 16
    assert len(L.sift_hip_verify_homography_host.argtypes) == 14
    assert len(L.sift_hip_score_homography_device.argtypes) == 15
    assert len(L.sift_hip_verify_homography_hypotheses_host.argtypes) == 5
    assert len(L.sift_hip_project_homography_device.argtypes) == 7
    assert "abi=1" in sift.version()
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    R = sift._HomographyResult
    assert layout == [ctypes.sizeof(R)] + [getattr(R, f).offset for f in RESULT_FIELDS] + [INVALID, STATE, 1]
    assert ctypes.sizeof(R) == 52 == sift.HOMOGRAPHY_RESULT_DTYPE.itemsize
    assert sift.HOMOGRAPHY_RESULT_DTYPE.names == RESULT_FIELDS
    assert [sift.HOMOGRAPHY_RESULT_DTYPE.fields[f][1] for f in RESULT_FIELDS] == [getattr(R, f).offset for f in RESULT_FIELDS]
    assert sift.HOMOGRAPHY_RESULT_DTYPE["H"].shape == (9,) and sift.HOMOGRAPHY_RESULT_DTYPE["H"].base == np.float32
    # the fundamental record is untouched
    assert ctypes.sizeof(sift._VerifyResult) == 52 and sift.VERIFY_RESULT_DTYPE.names[0] == "F"


def test_surfaces_exist(sift):
    from sift_amd import cv

    for name in ("verify_homography_device", "verify_homography_host", "score_homography_device",
                 "homography_hypotheses", "verify_device", "verify_host", "score_device", "hypotheses"):
        assert callable(getattr(sift.Verifier, name)), name
    for name in ("homography_samples", "homography_from_4", "transfer_inliers", "ransac_homography", "project_homography",
                 "homography_lstsq"):
        assert callable(getattr(cv, name)), name
    assert list(inspect.signature(cv.homography_samples).parameters) == ["n", "K", "seed"]
    assert list(inspect.signature(cv.ransac_samples).parameters) == ["n", "K", "seed"]
    assert list(inspect.signature(cv.transfer_inliers).parameters) == ["matches", "q_xy", "t_xy", "H", "max_error"]
    assert list(inspect.signature(cv.ransac_homography).parameters) == ["matches", "q_xy", "t_xy", "max_error", "K", "seed"]
    sig = inspect.signature(sift.verifyHomography).parameters
    assert (sig["max_error"].default, sig["hypotheses"].default, sig["seed"].default) == (1.5, 1024, 0)
    assert list(sig)[:5] == ["matches", "des_xy", "src_xy", "n_des", "n_src"]
    sig = inspect.signature(sift.project_homography_device).parameters
    assert list(sig) == ["H_ptr", "xy_ptr", "n", "out_ptr", "stride", "out_stride", "stream"]
    assert (sig["stride"].default, sig["out_stride"].default, sig["stream"].default) == (3, 2, None)
    # the device forms mirror the fundamental ones argument for argument
    assert list(inspect.signature(sift.Verifier.verify_homography_device).parameters) == \
        list(inspect.signature(sift.Verifier.verify_device).parameters)
    assert list(inspect.signature(sift.Verifier.verify_homography_host).parameters) == \
        list(inspect.signature(sift.Verifier.verify_host).parameters)
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::verifyHomography(std::vector<sift_cuda::DMatch" in out
    assert "sift_cuda::Verifier::verifyHomographyDevice(" in out and "sift_cuda::Verifier::verifyHomographyHost(" in out
    assert "sift_cuda::projectHomographyDevice(float const*, float const*, int, int, float*, int, void*)" in out
    assert "sift_cuda::verifyFundamental(std::vector<sift_cuda::DMatch" in out


class Calls:
    """The three entry points that take a list, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed 512-byte block in place of a verifier: limits 0

    def run(self, v="fake", matches=True, cap=4, qxy=True, qs=3, nq=4, txy=True, ts=3, nt=4, params="good", result=True,
            out="apart", K=16, max_error=1.5, H=True, counts=True):
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        prm = self.sift._VerifyParams(K, 0, max_error)
        pp = ctypes.byref(prm) if params == "good" else None
        res = self.sift._HomographyResult()
        mp, qp, tp = (p if matches else None), (p + 512 if qxy else None), (p + 512 if txy else None)
        op = {"apart": p + 768, "same": p, "overlap": p + 16 * max(cap - 1, 0), None: None}[out]
        got = [
            (L.sift_hip_verify_homography_device(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, pp, p + 640 if result else None,
                                                 op, None, None, None), L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_homography_host(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, pp,
                                               ctypes.byref(res) if result else None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_score_homography_device(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, p + 640 if H else None, K,
                                                max_error, p + 700 if counts else None, None),
             L.sift_hip_last_error().decode()),
        ]
        assert not self.buf.any() and not self.fake.any()
        assert bytes(res) == bytes(52)
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


def test_null_verifier_params_or_result(calls):
    for rc, msg in calls.run(v=None):
        assert rc == INVALID and "verifier" in msg, msg
    for rc, msg in calls.run(params=None)[:2]:
        assert rc == INVALID and "params" in msg, msg
    for rc, msg in calls.run(result=False)[:2]:
        assert rc == INVALID and "result" in msg, msg
    rc, msg = calls.run(H=False)[2]
    assert rc == INVALID and "null H" in msg, msg
    rc, msg = calls.run(counts=False)[2]
    assert rc == INVALID and "counts" in msg, msg


@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, cap):
    for rc, msg in calls.run(cap=cap):
        assert rc == INVALID and "cap" in msg, msg


def test_cap_over_the_verifiers_limit_is_refused(calls):
    for rc, msg in calls.run(cap=4, K=0):
        assert rc == INVALID and "hypotheses" in msg, msg
    for rc, msg in calls.run(cap=4):  # the stand-in's limits are 0
        assert rc == INVALID and ("hypotheses" in msg or "max_matches" in msg), msg
    for rc, msg in calls.run(cap=0, matches=False, qxy=False, txy=False, out=None):  # cap == 0 reaches the limits too
        assert rc == INVALID and "hypotheses" in msg, msg


@pytest.mark.parametrize("K", [0, -1, 4097])
def test_bad_hypotheses_is_refused(calls, K):
    for rc, msg in calls.run(K=K):
        assert rc == INVALID and "hypotheses" in msg, msg


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


@pytest.mark.parametrize("out", ["same", "overlap"])
def test_out_aliasing_matches_is_refused(calls, out):
    rc, msg = calls.run(out=out)[0]
    assert rc == INVALID and "alias" in msg, msg


def test_hypotheses_getters_refuse_a_verifier_without_a_call_of_their_model(calls):
    L, fake = calls.L, ctypes.c_void_p(calls.fake.ctypes.data)
    out = np.zeros(64, np.int32)
    for fn in (L.sift_hip_verify_homography_hypotheses_host, L.sift_hip_verify_hypotheses_host):
        assert fn(None, None, None, None, 4) == INVALID and b"verifier" in L.sift_hip_last_error()
        assert fn(fake, None, None, None, -1) == INVALID and b"cap" in L.sift_hip_last_error()
        assert fn(fake, out.ctypes.data, None, None, 4) == STATE and L.sift_hip_last_error()  # no verify call has run
    assert not out.any() and not calls.fake.any()


def project(sift, H=True, xy=0, stride=3, n=4, out=1024, out_stride=2, buf=None):
    """sift_hip_project_homography_device on offsets (bytes) into a host block; None: a null pointer."""
    L, p = sift.lib(), buf.ctypes.data
    at = lambda o: None if o is None else p + o  # noqa: E731
    rc = L.sift_hip_project_homography_device(p + 3072 if H else None, at(xy), stride, n, at(out), out_stride, None)
    assert not buf.any()
    return rc, L.sift_hip_last_error().decode()


def test_projection_refuses_bad_arguments(sift):
    buf = np.zeros(1024, np.int32)  # 4096 bytes, never touched: nothing is launched on a refusal
    rc, msg = project(sift, H=False, buf=buf)
    assert rc == INVALID and "null H" in msg, msg
    rc, msg = project(sift, H=False, n=0, buf=buf)  # also with nothing to do
    assert rc == INVALID and "null H" in msg, msg
    for kw in (dict(stride=1), dict(out_stride=1), dict(stride=0), dict(out_stride=-2)):
        rc, msg = project(sift, buf=buf, **kw)
        assert rc == INVALID and "stride" in msg, (kw, msg)
    rc, msg = project(sift, n=-1, buf=buf)
    assert rc == INVALID and "row count" in msg, msg
    for kw in (dict(xy=None), dict(out=None)):
        rc, msg = project(sift, buf=buf, **kw)
        assert rc == INVALID and "null position" in msg, (kw, msg)
    # n == 0 succeeds, with null positions too
    assert project(sift, n=0, buf=buf)[0] == 0 and project(sift, n=0, xy=None, out=None, buf=buf)[0] == 0
    # a partial overlap: shifted rows, the same start with other strides, the output's tail inside the input, the
    # input's last row inside the output
    for kw in (dict(xy=0, out=4, stride=2, out_stride=2), dict(xy=0, out=0, stride=3, out_stride=2),
               dict(xy=0, out=0, stride=2, out_stride=3), dict(xy=40, out=0, stride=3, out_stride=3),
               dict(xy=0, out=3 * 12, stride=3, out_stride=2), dict(xy=0, out=3 * 12 + 4, stride=3, out_stride=2)):
        rc, msg = project(sift, buf=buf, **kw)
        assert rc == INVALID and "overlap" in msg, (kw, msg)
    # a single row's extent is two floats: the third float of a stride-3 row is not part of it
    rc, msg = project(sift, xy=0, out=4, n=1, buf=buf)
    assert rc == INVALID and "overlap" in msg, msg
