"""Batched two-view verification (sift_hip_verifier_create_batched, sift_hip_verify_*_batched_*): what runs without a
GPU, after tests/test_verify_abi.py.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_verify_pair has the layout
  of its ctypes mirror.
* Creation refuses limits outside 1..64 x 65536 matches, 1..4096 hypotheses and 1..64 pairs before any device call.
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

import verify_batched_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
INVALID = -1  # SIFT_HIP_ERR_INVALID

NAMES = ("sift_hip_verifier_create_batched", "sift_hip_verify_fundamental_batched_device",
         "sift_hip_verify_fundamental_batched_host", "sift_hip_verify_homography_batched_device",
         "sift_hip_verify_homography_batched_host")
SIGNATURES = """
#include "sift_hip.h"
int (*a)(int, int, int, int, sift_hip_verifier_t*) = sift_hip_verifier_create_batched;
int (*b)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_verify_params*, sift_hip_verify_result*, sift_hip_dmatch*, int*, uint8_t*, void*) =
    sift_hip_verify_fundamental_batched_device;
int (*c)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_verify_params*, sift_hip_verify_result*, sift_hip_dmatch*, uint8_t*) =
    sift_hip_verify_fundamental_batched_host;
int (*d)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_verify_params*, sift_hip_homography_result*, sift_hip_dmatch*, int*, uint8_t*, void*) =
    sift_hip_verify_homography_batched_device;
int (*e)(sift_hip_verifier_t, const sift_hip_dmatch*, const int*, int, const sift_hip_verify_pair*, int, int,
         const sift_hip_verify_params*, sift_hip_homography_result*, sift_hip_dmatch*, uint8_t*) =
    sift_hip_verify_homography_batched_host;
int abi[SIFT_HIP_ABI_VERSION == 1 ? 1 : -1];
"""
PAIR_FIELDS = ("query_xy", "train_xy", "nq", "nt", "cap")
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_verify_pair), %s};
int main(void) {
    for (unsigned i = 0; i < sizeof layout / sizeof *layout; i++) printf("%%d\\n", layout[i]);
    return 0;
}
""" % ", ".join(f"__builtin_offsetof(sift_hip_verify_pair, {f})" for f in PAIR_FIELDS)


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
    assert len(L.sift_hip_verifier_create_batched.argtypes) == 5
    assert len(L.sift_hip_verify_fundamental_batched_device.argtypes) == 13
    assert len(L.sift_hip_verify_homography_batched_device.argtypes) == 13
    assert len(L.sift_hip_verify_fundamental_batched_host.argtypes) == 11
    assert len(L.sift_hip_verify_homography_batched_host.argtypes) == 11
    assert "abi=1" in sift.version()
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = sift._VerifyPair
    assert layout == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in PAIR_FIELDS]
    assert [f for f, _ in P._fields_] == list(PAIR_FIELDS)


def test_surfaces_exist(sift):
    from sift_amd import multi

    for name in ("verify_batched_device", "verify_homography_batched_device", "verify_batched_host",
                 "verify_homography_batched_host"):
        assert callable(getattr(sift.Verifier, name)), name
        sig = list(inspect.signature(getattr(sift.Verifier, name)).parameters)
        assert sig[:4] == ["self", "matches_ptr", "counts_ptr", "pairs"], sig
    init = inspect.signature(sift.Verifier.__init__).parameters
    assert list(init)[:4] == ["self", "max_matches", "max_hypotheses", "max_pairs"]
    assert init["max_pairs"].default == 1 and init["max_hypotheses"].default == 1024
    for name in ("verifyFundamentalBatched", "verifyHomographyBatched"):
        sig = inspect.signature(getattr(sift, name)).parameters
        assert list(sig)[:2] == ["matches_per_pair", "xy_per_pair"]
        assert (sig["max_error"].default, sig["hypotheses"].default, sig["seed"].default) == (1.5, 1024, 0)
    assert list(inspect.signature(multi.position_pairs).parameters) == ["gathered_xy", "counts", "rank", "world"]
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::Verifier::Verifier(int, int, int, int)" in out
    assert "sift_cuda::Verifier::Verifier(int, int, int)" in out  # the existing constructor is still there
    for name in ("verifyBatchedDevice", "verifyHomographyBatchedDevice", "verifyBatchedHost",
                 "verifyHomographyBatchedHost"):
        assert f"sift_cuda::Verifier::{name}(sift_cuda::DMatch const*, int const*, std::vector<sift_cuda::VerifyPair" in out
    header = open(os.path.join(ROOT, "include", "sift_cuda", "Verify.hh")).read()
    assert "std::vector<TwoViewGeometry> verifyBatchedHost(" in header
    assert "std::vector<PlanarGeometry> verifyHomographyBatchedHost(" in header


@pytest.mark.parametrize("limits", [(0, 64, 4), (-1, 64, 4), (64 * 65536 + 1, 64, 4), (100, 0, 4), (100, 4097, 4),
                                    (100, 64, 0), (100, 64, -1), (100, 64, 65)])
def test_create_refuses_bad_limits(sift, limits):
    L = sift.lib()
    v = ctypes.c_void_p(1)
    assert L.sift_hip_verifier_create_batched(0, *limits, ctypes.byref(v)) == INVALID
    assert b"limits" in L.sift_hip_last_error()
    assert L.sift_hip_verifier_create_batched(0, 100, 64, 4, None) == INVALID
    with pytest.raises(sift.SiftHipError):
        sift.Verifier(*limits)
    # the plain creation keeps its own range of max_matches
    assert L.sift_hip_verifier_create(0, 65537, 64, ctypes.byref(v)) == INVALID


def test_create_without_a_device_is_a_status(sift):
    L = sift.lib()
    n = ctypes.c_int(-1)
    if L.sift_hip_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is visible")
    v = ctypes.c_void_p(1)
    assert L.sift_hip_verifier_create_batched(0, 64 * 65536, 64, 64, ctypes.byref(v)) < 0 and not v.value
    assert L.sift_hip_last_error()


class Calls:
    """The four batched entry points, on host memory that must never be touched."""

    def __init__(self, sift):
        self.sift, self.L = sift, sift.lib()
        self.buf = np.zeros(256, np.int32)
        self.fake = np.zeros(64, np.int64)  # a zeroed block in place of a verifier: limits 0

    def run(self, v="fake", matches=True, P=2, pairs="good", caps=(4, 3), qxy=True, txy=True, nq=4, nt=4, qs=3, ts=3,
            params="good", result=True, out="apart", K=16, max_error=1.5):
        L, p = self.L, self.buf.ctypes.data
        vp = {"fake": ctypes.c_void_p(self.fake.ctypes.data), None: None}[v]
        prm = self.sift._VerifyParams(K, 0, max_error)
        pp = ctypes.byref(prm) if params == "good" else None
        table = (self.sift._VerifyPair * max(len(caps), 1))(
            *[self.sift._VerifyPair(p + 512 if qxy else None, p + 512 if txy else None, nq, nt, c) for c in caps])
        tp = table if pairs == "good" else None
        mp = p if matches else None
        rows = sum(c for c in caps if 0 < c <= 65536)
        op = {"apart": p + 768, "same": p, "overlap": p + 16 * max(rows - 1, 0), None: None}[out]
        rp = p + 640 if result else None
        got = []
        for name in ("fundamental", "homography"):
            dev = getattr(L, f"sift_hip_verify_{name}_batched_device")
            host = getattr(L, f"sift_hip_verify_{name}_batched_host")
            got.append((dev(vp, mp, None, P, tp, qs, ts, pp, rp, op, None, None, None), L.sift_hip_last_error().decode()))
            got.append((host(vp, mp, None, P, tp, qs, ts, pp, rp, None, None), L.sift_hip_last_error().decode()))
        assert not self.buf.any() and not self.fake.any()
        return got


@pytest.fixture(scope="module")
def calls(sift):
    return Calls(sift)


def test_null_verifier_pairs_params_or_results(calls):
    for rc, msg in calls.run(v=None):
        assert rc == INVALID and "verifier" in msg, msg
    for rc, msg in calls.run(pairs=None):
        assert rc == INVALID and "pairs" in msg, msg
    for rc, msg in calls.run(params=None):
        assert rc == INVALID and "params" in msg, msg
    for rc, msg in calls.run(result=False):
        assert rc == INVALID and "result" in msg, msg


@pytest.mark.parametrize("P", [0, -1, 65, 2 ** 31 - 1])
def test_bad_pair_count_is_refused(calls, P):
    for rc, msg in calls.run(P=P):
        assert rc == INVALID and "pairs outside" in msg, msg


def test_more_pairs_than_the_verifier_holds_is_refused(calls):
    for rc, msg in calls.run(P=1, caps=(4,)):  # the stand-in's limits are 0: hypotheses, then pairs, then rows
        assert rc == INVALID and "hypotheses" in msg, msg


@pytest.mark.parametrize("cap", [-1, 65537, 2 ** 31 - 1])
def test_bad_cap_is_refused(calls, cap):
    for caps in ((cap, 4), (4, cap)):
        for rc, msg in calls.run(caps=caps):
            assert rc == INVALID and "cap" in msg and "pair %d" % caps.index(cap) in msg, msg


def test_spill_caps_are_refused(calls):
    """SPILL: a cap of 70 000 is refused as a cap wherever it stands, before the sum is looked at."""
    for caps in (bc.SPILL["caps"], bc.SPILL["caps"][::-1]):
        for rc, msg in calls.run(caps=caps):
            assert rc == INVALID and "cap must lie in 0..65536" in msg, msg
    for rc, msg in calls.run(caps=(65536, 65536), out=None):  # both in range: the stand-in's limits refuse the call
        assert rc == INVALID and ("hypotheses" in msg or "max_matches" in msg or "max_pairs" in msg), msg


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


def test_null_pointers_and_negative_row_counts_are_refused(calls):
    for rc, msg in calls.run(matches=False):
        assert rc == INVALID and "matches" in msg, msg
    for kw in (dict(qxy=False), dict(txy=False)):
        for rc, msg in calls.run(**kw):
            assert rc == INVALID and "position" in msg, msg
    for kw in (dict(nq=-1), dict(nt=-1)):
        for rc, msg in calls.run(**kw):
            assert rc == INVALID and "row count" in msg, msg
    # null positions and null matches are fine where no row exists: such a call reaches the stand-in's limits
    for rc, msg in calls.run(matches=False, qxy=False, txy=False, caps=(0, 0)):
        assert rc == INVALID and "hypotheses" in msg, msg


@pytest.mark.parametrize("out", ["same", "overlap"])
def test_out_aliasing_matches_is_refused(calls, out):
    got = calls.run(out=out)
    for rc, msg in (got[0], got[2]):  # the device forms
        assert rc == INVALID and "alias" in msg, msg
