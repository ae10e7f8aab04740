"""Two-view verification (sift_hip_verifier_*, sift_hip_verify_*, sift_hip_score_*): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_verify_params and
  sift_hip_verify_result have the layout of their ctypes mirrors; the defaults are 1024 hypotheses, seed 0, 1.5 px.
* Creation refuses limits outside 1..65536 matches and 1..4096 hypotheses before any device call, and without a device
  fails with a status (no crash).
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, and nothing is launched: the
  calls run on host memory that is never read or written and on a verifier that is null, or a zeroed block standing
  in for one (limits 0: whatever reaches the limit rules is refused there, still before any device call).
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
INVALID = -1  # SIFT_HIP_ERR_INVALID

NAMES = ("sift_hip_default_verify_params", "sift_hip_verifier_create", "sift_hip_verifier_destroy",
         "sift_hip_verify_fundamental_device", "sift_hip_verify_fundamental_host", "sift_hip_score_fundamental_device",
         "sift_hip_verify_hypotheses_host")
SIGNATURES = """
#include "sift_hip.h"
void (*a)(sift_hip_verify_params*) = sift_hip_default_verify_params;
int (*b)(int, int, int, sift_hip_verifier_t*) = sift_hip_verifier_create;
int (*c)(sift_hip_verifier_t) = sift_hip_verifier_destroy;
int (*d)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_verify_params*, sift_hip_verify_result*, sift_hip_dmatch*, int*, uint8_t*, void*) =
    sift_hip_verify_fundamental_device;
int (*e)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const sift_hip_verify_params*, sift_hip_verify_result*, sift_hip_dmatch*, uint8_t*) =
    sift_hip_verify_fundamental_host;
int (*f)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const float*, int, int, const float*, int, int,
         const float*, int, float, int*, void*) = sift_hip_score_fundamental_device;
int (*g)(sift_hip_verifier_t, int*, float*, int*, int) = sift_hip_verify_hypotheses_host;
"""
PARAM_FIELDS = ("hypotheses", "seed", "max_error")
RESULT_FIELDS = ("F", "inliers", "hypothesis", "matches", "valid_hypotheses")
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_verify_params), %s, sizeof(sift_hip_verify_result), %s};
int main(void) {
    sift_hip_verify_params p = {1024, 0u, 1.5f};
    (void)p;
    for (unsigned i = 0; i < sizeof layout / sizeof *layout; i++) printf("%%d\\n", layout[i]);
    return 0;
}
""" % (", ".join(f"__builtin_offsetof(sift_hip_verify_params, {f})" for f in PARAM_FIELDS),
       ", ".join(f"__builtin_offsetof(sift_hip_verify_result, {f})" for f in RESULT_FIELDS))


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
    assert len(L.sift_hip_verify_fundamental_device.argtypes) == 16
    assert len(L.sift_hip_verify_fundamental_host.argtypes) == 14
    assert len(L.sift_hip_score_fundamental_device.argtypes) == 15
    assert len(L.sift_hip_verify_hypotheses_host.argtypes) == 5
    assert "abi=1" in sift.version()
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, R = sift._VerifyParams, sift._VerifyResult
    assert layout == ([ctypes.sizeof(P)] + [getattr(P, f).offset for f in PARAM_FIELDS]
                      + [ctypes.sizeof(R)] + [getattr(R, f).offset for f in RESULT_FIELDS])
    assert ctypes.sizeof(R) == 52 == sift.VERIFY_RESULT_DTYPE.itemsize
    assert [sift.VERIFY_RESULT_DTYPE.fields[f][1] for f in RESULT_FIELDS] == [getattr(R, f).offset for f in RESULT_FIELDS]


def test_defaults(sift):
    p = sift._VerifyParams(-1, 7, -1.0)
    sift.lib().sift_hip_default_verify_params(ctypes.byref(p))
    assert (p.hypotheses, p.seed, p.max_error) == (1024, 0, 1.5)
    sift.lib().sift_hip_default_verify_params(None)  # a no-op
    sig = inspect.signature(sift.verifyFundamental).parameters
    assert (sig["max_error"].default, sig["hypotheses"].default, sig["seed"].default) == (1.5, 1024, 0)
    assert list(sig)[:5] == ["matches", "des_xy", "src_xy", "n_des", "n_src"]
    assert inspect.signature(sift.Verifier.__init__).parameters["max_hypotheses"].default == 1024


def test_surfaces_exist(sift):
    from sift_amd import cv

    for name in ("verify_device", "verify_host", "score_device", "hypotheses"):
        assert callable(getattr(sift.Verifier, name)), name
    for name in ("ransac_samples", "fundamental_from_8", "sampson_inliers", "ransac_fundamental", "fundamental_lstsq"):
        assert callable(getattr(cv, name)), name
    assert list(inspect.signature(cv.ransac_samples).parameters) == ["n", "K", "seed"]
    assert list(inspect.signature(cv.sampson_inliers).parameters) == ["matches", "q_xy", "t_xy", "F", "max_error"]
    assert list(inspect.signature(cv.ransac_fundamental).parameters) == ["matches", "q_xy", "t_xy", "max_error", "K",
                                                                         "seed"]
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::verifyFundamental(std::vector<sift_cuda::DMatch" in out
    assert "sift_cuda::Verifier::Verifier(int, int, int)" in out
    assert "sift_cuda::Verifier::verifyDevice(" in out and "sift_cuda::Verifier::verifyHost(" in out


@pytest.mark.parametrize("max_matches,max_hypotheses", [(0, 64), (-1, 64), (65537, 64), (100, 0), (100, -5), (100, 4097)])
def test_create_refuses_bad_limits(sift, max_matches, max_hypotheses):
    L = sift.lib()
    v = ctypes.c_void_p(1)
    assert L.sift_hip_verifier_create(0, max_matches, max_hypotheses, ctypes.byref(v)) == INVALID
    assert b"limits" in L.sift_hip_last_error()
    assert L.sift_hip_verifier_create(0, 100, 64, None) == INVALID
    with pytest.raises(sift.SiftHipError):
        sift.Verifier(max_matches, max_hypotheses)


def test_create_without_a_device_is_a_status(sift):
    L = sift.lib()
    n = ctypes.c_int(-1)
    if L.sift_hip_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is visible")
    v = ctypes.c_void_p(1)
    assert L.sift_hip_verifier_create(0, 100, 64, ctypes.byref(v)) < 0 and not v.value
    assert L.sift_hip_last_error()
    assert L.sift_hip_verifier_destroy(None) == 0  # like free(NULL)


class Calls:
    """The three entry points that take a list, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed block in place of a verifier: limits 0

    def run(self, v="fake", matches=True, cap=4, qxy=True, qs=3, nq=4, txy=True, ts=3, nt=4, params="good", result=True,
            out="apart", K=16, max_error=1.5):
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        prm = self.sift._VerifyParams(K, 0, max_error)
        pp = ctypes.byref(prm) if params == "good" else None
        res = self.sift._VerifyResult()
        mp, qp, tp = (p if matches else None), (p + 512 if qxy else None), (p + 512 if txy else None)
        op = {"apart": p + 768, "same": p, "overlap": p + 16 * max(cap - 1, 0), None: None}[out]
        got = [
            (L.sift_hip_verify_fundamental_device(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, pp, p + 640 if result else None,
                                                  op, None, None, None), L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_fundamental_host(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, pp,
                                                ctypes.byref(res) if result else None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_score_fundamental_device(vp, mp, None, cap, qp, qs, nq, tp, ts, nt, p + 640, K, max_error,
                                                 p + 700, None), L.sift_hip_last_error().decode()),
        ]
        assert not self.buf.any() and not self.fake.any()
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
    L = calls.L
    assert L.sift_hip_verify_hypotheses_host(None, None, None, None, 4) == INVALID
    assert L.sift_hip_score_fundamental_device(ctypes.c_void_p(calls.fake.ctypes.data), calls.buf.ctypes.data, None, 4,
                                               calls.buf.ctypes.data, 3, 4, calls.buf.ctypes.data, 3, 4, None, 4, 1.5,
                                               calls.buf.ctypes.data, None) == INVALID  # null F


@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, cap):
    for rc, msg in calls.run(cap=cap):
        assert rc == INVALID and "cap" in msg, msg


def test_cap_over_the_verifiers_limit_is_refused(calls):
    for rc, msg in calls.run(cap=4, K=0):
        assert rc == INVALID and "hypotheses" in msg, msg
    for rc, msg in calls.run(cap=4):  # the stand-in's limits are 0
        assert rc == INVALID and ("hypotheses" in msg or "max_matches" in msg), msg


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
