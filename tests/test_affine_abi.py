"""Affine and similarity verification (sift_hip_verify_affine_*, sift_hip_score_affine_device,
sift_hip_refine_affine_*): what runs without a GPU, after tests/test_homography_abi.py.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_affine_result is the
  homography's 52-byte record; the model constants are 0 and 1; the ABI version is still 1.
* Every argument the header lists as invalid is SIFT_HIP_ERR_INVALID with a message, and nothing is launched: the
  calls run on host memory that is never read or written and on a verifier that is null, or a zeroed block standing
  in for one (limits 0: whatever reaches the limit rules is refused there, still before any device call).  A model
  that is neither constant is refused as well.
* The hypotheses getter refuses a verifier no verify call of its model has run on.
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

ARGS = {"sift_hip_verify_affine_device": 17, "sift_hip_verify_affine_host": 15, "sift_hip_score_affine_device": 15,
        "sift_hip_verify_affine_hypotheses_host": 6, "sift_hip_verify_affine_batched_device": 14,
        "sift_hip_verify_affine_batched_host": 12, "sift_hip_refine_affine_device": 19, "sift_hip_refine_affine_host": 18,
        "sift_hip_refine_affine_batched_device": 16, "sift_hip_refine_affine_batched_host": 15}
SIGNATURES = """
#include "sift_hip.h"
#define ONE const int*, int, const float*, int, int, const float*, int, int
#define MANY const int*, int, const sift_hip_verify_pair*, int, int
int (*a)(sift_hip_verifier_t, int, const sift_hip_dmatch*, ONE, const sift_hip_verify_params*, sift_hip_affine_result*,
         sift_hip_dmatch*, int*, uint8_t*, void*) = sift_hip_verify_affine_device;
int (*b)(sift_hip_verifier_t, int, const sift_hip_dmatch*, ONE, const sift_hip_verify_params*, sift_hip_affine_result*,
         sift_hip_dmatch*, uint8_t*) = sift_hip_verify_affine_host;
int (*c)(sift_hip_verifier_t, const sift_hip_dmatch*, ONE, const float*, int, float, int*, void*) =
    sift_hip_score_affine_device;
int (*d)(sift_hip_verifier_t, int, int*, float*, int*, int) = sift_hip_verify_affine_hypotheses_host;
int (*e)(sift_hip_verifier_t, int, const sift_hip_dmatch*, MANY, const sift_hip_verify_params*, sift_hip_affine_result*,
         sift_hip_dmatch*, int*, uint8_t*, void*) = sift_hip_verify_affine_batched_device;
int (*f)(sift_hip_verifier_t, int, const sift_hip_dmatch*, MANY, const sift_hip_verify_params*, sift_hip_affine_result*,
         sift_hip_dmatch*, uint8_t*) = sift_hip_verify_affine_batched_host;
int (*g)(sift_hip_verifier_t, int, const sift_hip_dmatch*, ONE, float, int, sift_hip_affine_result*, uint8_t*,
         sift_hip_dmatch*, int*, int*, void*) = sift_hip_refine_affine_device;
int (*h)(sift_hip_verifier_t, int, const sift_hip_dmatch*, ONE, float, int, sift_hip_affine_result*, uint8_t*,
         sift_hip_dmatch*, int*, int*) = sift_hip_refine_affine_host;
int (*i)(sift_hip_verifier_t, int, const sift_hip_dmatch*, MANY, float, int, sift_hip_affine_result*, uint8_t*,
         sift_hip_dmatch*, int*, int*, void*) = sift_hip_refine_affine_batched_device;
int (*j)(sift_hip_verifier_t, int, const sift_hip_dmatch*, MANY, float, int, sift_hip_affine_result*, uint8_t*,
         sift_hip_dmatch*, int*, int*) = sift_hip_refine_affine_batched_host;
sift_hip_homography_result* same_type(sift_hip_affine_result* r) { return r; }
"""
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_affine_result), sizeof(sift_hip_homography_result), SIFT_HIP_MODEL_AFFINE,
                SIFT_HIP_MODEL_SIMILARITY, SIFT_HIP_ERR_INVALID, SIFT_HIP_ERR_STATE, SIFT_HIP_ABI_VERSION};
int main(void) {
    for (unsigned i = 0; i < sizeof layout / sizeof *layout; i++) printf("%d\\n", layout[i]);
    return 0;
}
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
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert layout == [52, 52, 0, 1, INVALID, STATE, 1]
    assert sift.AFFINE_RESULT_DTYPE is sift.HOMOGRAPHY_RESULT_DTYPE and sift.AFFINE_RESULT_DTYPE.itemsize == 52
    assert (sift.MODEL_AFFINE, sift.MODEL_SIMILARITY) == (0, 1)
    # the other models' records are untouched
    assert ctypes.sizeof(sift._VerifyResult) == 52 and ctypes.sizeof(sift._HomographyResult) == 52


def test_surfaces_exist(sift):
    from sift_amd import cv

    V = sift.Verifier
    for name, twin in (("verify_affine_device", "verify_homography_device"), ("verify_affine_host", "verify_homography_host"),
                       ("score_affine_device", "score_homography_device"),
                       ("verify_affine_batched_device", "verify_homography_batched_device"),
                       ("verify_affine_batched_host", "verify_homography_batched_host"),
                       ("refine_affine_device", "refine_homography_device"), ("refine_affine_host", "refine_homography_host"),
                       ("refine_affine_batched_device", "refine_homography_batched_device"),
                       ("refine_affine_batched_host", "refine_homography_batched_host")):
        got = inspect.signature(getattr(V, name)).parameters
        want = list(inspect.signature(getattr(V, twin)).parameters)
        # the homography form argument for argument (the score's matrix is A), then similarity = False
        assert [p.replace("A_ptr", "H_ptr") for p in got] == want + ["similarity"], name
        assert got["similarity"].default is False, name
    assert list(inspect.signature(V.affine_hypotheses).parameters) == ["self", "similarity"]
    for name in ("affine_samples", "similarity_samples", "affine_from_3", "similarity_from_2", "affine_inliers",
                 "ransac_affine", "refit_affine", "refine_affine", "affine_lstsq"):
        assert callable(getattr(cv, name)), name
    assert list(inspect.signature(cv.ransac_affine).parameters) == ["matches", "q_xy", "t_xy", "max_error", "K", "seed",
                                                                    "similarity"]
    assert list(inspect.signature(cv.affine_lstsq).parameters) == ["q_pts", "t_pts", "similarity"]
    for fn, twin in ((sift.verifyAffine, sift.verifyHomography), (sift.verifyAffineBatched, sift.verifyHomographyBatched)):
        sig, want = inspect.signature(fn).parameters, inspect.signature(twin).parameters
        assert set(sig) == set(want) | {"similarity"} and sig["similarity"].default is False
        assert all(sig[k].default == want[k].default for k in want)
    assert list(inspect.signature(sift.verifyAffine).parameters)[:6] == ["matches", "des_xy", "src_xy", "n_des", "n_src",
                                                                         "similarity"]
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::verifyAffine(std::vector<sift_cuda::DMatch" in out
    for name in ("verifyAffineDevice", "verifyAffineHost", "verifyAffineBatchedDevice", "verifyAffineBatchedHost",
                 "refineAffineDevice", "refineAffineHost", "refineAffineBatchedDevice", "refineAffineBatchedHost"):
        assert "sift_cuda::Verifier::%s(" % name in out, name


class Calls:
    """The entry points that take one list, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed 512-byte block in place of a verifier: limits 0

    def run(self, v="fake", model=0, matches=True, cap=4, qxy=True, qs=3, nq=4, txy=True, ts=3, nt=4, params="good",
            result=True, out="apart", K=16, max_error=1.5, A=True, counts=True, rounds=1, mask=True):
        """(rc, message) of verify_device, verify_host, refine_device, refine_host and score_device."""
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        prm = self.sift._VerifyParams(K, 0, max_error)
        pp = ctypes.byref(prm) if params == "good" else None
        res = self.sift._HomographyResult()
        mp, qp, tp = (p if matches else None), (p + 512 if qxy else None), (p + 512 if txy else None)
        op = {"apart": p + 768, "same": p, "overlap": p + 16 * max(cap - 1, 0), None: None}[out]
        rp, kp = (p + 640 if result else None), (p + 720 if mask else None)
        lst = (mp, None, cap, qp, qs, nq, tp, ts, nt)
        got = [
            (L.sift_hip_verify_affine_device(vp, model, *lst, pp, rp, op, None, None, None), L.sift_hip_last_error().decode()),
            (L.sift_hip_verify_affine_host(vp, model, *lst, pp, ctypes.byref(res) if result else None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_refine_affine_device(vp, model, *lst, max_error, rounds, rp, kp, op, None, None, None),
             L.sift_hip_last_error().decode()),
            (L.sift_hip_refine_affine_host(vp, model, *lst, max_error, rounds, ctypes.byref(res) if result else None, kp,
                                           None, None, None), L.sift_hip_last_error().decode()),
            (L.sift_hip_score_affine_device(vp, *lst, p + 640 if A else None, K, max_error, p + 700 if counts else None,
                                            None), L.sift_hip_last_error().decode()),
        ]
        assert not self.buf.any() and not self.fake.any()
        assert bytes(res) == bytes(52)
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


@pytest.mark.parametrize("model", [0, 1])
def test_null_verifier_params_or_result(calls, model):
    for rc, msg in calls.run(v=None, model=model):
        assert rc == INVALID and "verifier" in msg, msg
    for rc, msg in calls.run(params=None, model=model)[:2]:
        assert rc == INVALID and "params" in msg, msg
    for rc, msg in calls.run(result=False, model=model)[:4]:
        assert rc == INVALID and "result" in msg, msg
    rc, msg = calls.run(A=False)[4]
    assert rc == INVALID and "null A" in msg, msg
    rc, msg = calls.run(counts=False)[4]
    assert rc == INVALID and "counts" in msg, msg


@pytest.mark.parametrize("model", [-1, 2, 3, 2 ** 31 - 1])
def test_a_model_that_is_neither_constant_is_refused(calls, model):
    for rc, msg in calls.run(model=model)[:4]:
        assert rc == INVALID and "model" in msg, msg
    L, fake = calls.L, ctypes.c_void_p(calls.fake.ctypes.data)
    assert L.sift_hip_verify_affine_hypotheses_host(fake, model, None, None, None, 4) == INVALID
    assert b"model" in L.sift_hip_last_error()
    table = (calls.sift._VerifyPair * 1)(calls.sift._VerifyPair(None, None, 0, 0, 0))
    prm = calls.sift._VerifyParams(16, 0, 1.5)
    p = calls.buf.ctypes.data
    for rc in (L.sift_hip_verify_affine_batched_device(fake, model, None, None, 1, table, 3, 3, ctypes.byref(prm), p, None,
                                                       None, None, None),
               L.sift_hip_verify_affine_batched_host(fake, model, None, None, 1, table, 3, 3, ctypes.byref(prm), p, None, None),
               L.sift_hip_refine_affine_batched_device(fake, model, None, None, 1, table, 3, 3, 1.5, 1, p, None, None, None,
                                                       None, None),
               L.sift_hip_refine_affine_batched_host(fake, model, None, None, 1, table, 3, 3, 1.5, 1, p, None, None, None,
                                                     None)):
        assert rc == INVALID and b"model" in L.sift_hip_last_error()
    assert not calls.buf.any() and not calls.fake.any()


@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, cap):
    for rc, msg in calls.run(cap=cap):
        assert rc == INVALID and "cap" in msg, msg


def test_cap_over_the_verifiers_limit_is_refused(calls):
    for rc, msg in calls.run(cap=4):  # the stand-in's limits are 0
        assert rc == INVALID and ("hypotheses" in msg or "max_matches" in msg), msg
    for rc, msg in calls.run(cap=0, matches=False, qxy=False, txy=False, out=None, mask=False):  # cap == 0 reaches them too
        assert rc == INVALID and "hypotheses" in msg, msg


@pytest.mark.parametrize("K", [0, -1, 4097])
def test_bad_hypotheses_is_refused(calls, K):
    got = calls.run(K=K)
    for rc, msg in got[:2] + got[4:]:
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
    got = calls.run(out=out)
    for rc, msg in (got[0], got[2]):
        assert rc == INVALID and "alias" in msg, msg


def test_refine_refuses_a_null_mask_and_bad_rounds(calls):
    for rc, msg in calls.run(mask=False)[2:4]:
        assert rc == INVALID and "mask" in msg, msg
    for rounds in (0, -1, 9):
        for rc, msg in calls.run(rounds=rounds)[2:4]:
            assert rc == INVALID and "rounds" in msg, msg


def test_hypotheses_getter_refuses_a_verifier_without_a_call_of_its_model(calls):
    L, fake = calls.L, ctypes.c_void_p(calls.fake.ctypes.data)
    out = np.zeros(64, np.int32)
    fn = L.sift_hip_verify_affine_hypotheses_host
    for model in (0, 1):
        assert fn(None, model, None, None, None, 4) == INVALID and b"verifier" in L.sift_hip_last_error()
        assert fn(fake, model, None, None, None, -1) == INVALID and b"cap" in L.sift_hip_last_error()
        assert fn(fake, model, out.ctypes.data, None, None, 4) == STATE and L.sift_hip_last_error()  # no verify call has run
    assert not out.any() and not calls.fake.any()
