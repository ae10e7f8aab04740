"""k nearest neighbours (sift_hip_match_knn_*, knnMatch, matchKnnList): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents.
* The refusals that need no matcher -- k outside 1..SIFT_HIP_KNN_MAX, a NaN max_distance, a null matcher, for the
  host list a null count -- return SIFT_HIP_ERR_INVALID with a message naming them, before any device call (there is
  no device here).  The refusals that need a matcher's limits are in tests/test_gpu_match_knn.py.
* sift_hip_match_knn_plan answers on the host.
"""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")

SIGNATURES = """
#include "sift_hip.h"
_Static_assert(SIFT_HIP_KNN_MAX == 8, "two kernel instantiations: 4 and 8 entries");
_Static_assert(SIFT_HIP_ABI_VERSION == 1, "additions only");
int (*a)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, int, int*, float*, void*) = sift_hip_match_knn_device;
int (*b)(sift_hip_matcher_t, int, const uint16_t* const*, const int*, const uint16_t* const*, const int*, int, int*, float*,
         void*) = sift_hip_match_knn_batched;
int (*c)(sift_hip_matcher_t, const int8_t*, const int*, int, const int*, const int*, const int*, const int*, const int*,
         const int*, int, int*, float*, void*) = sift_hip_match_knn_codes_batched;
int (*d)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, int, int*, float*) = sift_hip_match_knn_host;
int (*e)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, int, float, sift_hip_dmatch*, int*, void*) =
    sift_hip_match_knn_list_device;
int (*f)(sift_hip_matcher_t, int, const uint16_t* const*, const int*, const uint16_t* const*, const int*, int, float,
         sift_hip_dmatch*, int*, void*) = sift_hip_match_knn_list_batched;
int (*g)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, int, float, sift_hip_dmatch*, int, int*) =
    sift_hip_match_knn_list_host;
int (*h)(int, int, int, int, int*) = sift_hip_match_knn_plan;
"""
NAMES = {"sift_hip_match_knn_device": 9, "sift_hip_match_knn_batched": 10, "sift_hip_match_knn_codes_batched": 14,
         "sift_hip_match_knn_host": 8, "sift_hip_match_knn_list_device": 10, "sift_hip_match_knn_list_batched": 11,
         "sift_hip_match_knn_list_host": 10, "sift_hip_match_knn_plan": 5}
INVALID = -1


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name, nargs in NAMES.items():
        assert name in exported, name
        assert len(getattr(sift.lib(), name).argtypes) == nargs, name
    src = tmp_path / "signatures.c"
    src.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv

    assert sift.KNN_MAX == cv.KNN_MAX == 8
    for name in ("match_knn_device", "match_knn_batched", "match_knn_codes_batched", "match_knn_host",
                 "match_knn_list_device", "match_knn_list_batched", "match_knn_list_host", "knn_plan"):
        assert callable(getattr(sift.Matcher, name)), name
    assert list(inspect.signature(sift.knnMatch).parameters) == ["des", "num_des", "src", "num_src", "k"]
    assert list(inspect.signature(sift.matchKnnList).parameters) == ["des", "num_des", "src", "num_src", "k", "max_distance"]
    assert callable(cv.knn) and callable(cv.knn_records)
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::matchKnn(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, int)" in out
    assert "sift_cuda::matchKnnList(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, int, float)" in out
    assert "sift_cuda::matchKnnBatchedDevice(" in out and "sift_cuda::matchKnnListBatchedDevice(" in out


def test_refusals_that_need_no_matcher(sift):
    L = sift.lib()
    buf = np.full(64, -7, np.int32)
    p = buf.ctypes.data
    pp = ctypes.c_void_p(p)
    one = ctypes.c_int(1)
    n = ctypes.c_int(-7)
    fake = ctypes.c_void_p(p)  # never dereferenced: k and max_distance are judged first

    def refused(rc, word):
        msg = L.sift_hip_last_error().decode()
        assert rc == INVALID and word in msg, (rc, msg, word)

    for k in (0, -1, 9):
        refused(L.sift_hip_match_knn_device(fake, p, 1, p, 1, k, p, p, None), "k outside")
        refused(L.sift_hip_match_knn_batched(fake, 1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp),
                                             ctypes.byref(one), k, p, p, None), "k outside")
        refused(L.sift_hip_match_knn_codes_batched(fake, p, p, 1, ctypes.byref(one), ctypes.byref(one), ctypes.byref(one),
                                                   ctypes.byref(one), ctypes.byref(one), ctypes.byref(one), k, p, p, None),
                "k outside")
        refused(L.sift_hip_match_knn_host(fake, p, 1, p, 1, k, p, p), "k outside")
        refused(L.sift_hip_match_knn_list_device(fake, p, 1, p, 1, k, 0.0, p, p, None), "k outside")
        refused(L.sift_hip_match_knn_list_batched(fake, 1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp),
                                                  ctypes.byref(one), k, 0.0, p, p, None), "k outside")
        refused(L.sift_hip_match_knn_list_host(fake, p, 1, p, 1, k, 0.0, p, 1, ctypes.byref(n)), "k outside")
        refused(L.sift_hip_match_knn_plan(10, 10, 1, k, ctypes.byref(n)), "k-NN shape")
    nan = float("nan")
    refused(L.sift_hip_match_knn_list_device(fake, p, 1, p, 1, 2, nan, p, p, None), "NaN")
    refused(L.sift_hip_match_knn_list_batched(fake, 1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp),
                                              ctypes.byref(one), 2, nan, p, p, None), "NaN")
    refused(L.sift_hip_match_knn_list_host(fake, p, 1, p, 1, 2, nan, p, 1, ctypes.byref(n)), "NaN")
    # a null matcher
    refused(L.sift_hip_match_knn_device(None, p, 1, p, 1, 2, p, p, None), "null matcher")
    refused(L.sift_hip_match_knn_batched(None, 1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp),
                                         ctypes.byref(one), 2, p, p, None), "null matcher")
    refused(L.sift_hip_match_knn_codes_batched(None, p, p, 1, ctypes.byref(one), ctypes.byref(one), ctypes.byref(one),
                                               ctypes.byref(one), ctypes.byref(one), ctypes.byref(one), 2, p, p, None),
            "null matcher")
    refused(L.sift_hip_match_knn_host(None, p, 1, p, 1, 2, p, p), "null matcher")
    refused(L.sift_hip_match_knn_list_device(None, p, 1, p, 1, 2, 0.0, p, p, None), "null matcher")
    refused(L.sift_hip_match_knn_list_batched(None, 1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp),
                                              ctypes.byref(one), 2, 0.0, p, p, None), "null matcher")
    refused(L.sift_hip_match_knn_list_host(None, p, 1, p, 1, 2, 0.0, p, 1, ctypes.byref(n)), "null matcher")
    refused(L.sift_hip_match_knn_list_host(None, p, 1, p, 1, 2, 0.0, p, 1, None), "null out or count")
    assert n.value == 0  # the host list's count is cleared, nothing else is written
    assert (buf == -7).all()


def test_plan_answers_on_the_host(sift):
    L = sift.lib()
    S = ctypes.c_int(-1)
    assert L.sift_hip_match_knn_plan(300, 256, 1, 8, ctypes.byref(S)) == 0 and S.value == 1  # one key group
    assert L.sift_hip_match_knn_plan(300, 257, 1, 8, ctypes.byref(S)) == 0 and S.value == 2
    assert sift.Matcher.knn_plan(300, 1100, 1, 3) == sift.Matcher.knn_plan(300, 1100, 1, 8) == 5  # whole key groups
    assert sift.Matcher.knn_plan(2000, 100000, 1) == 8  # at most 8 splits
    assert sift.Matcher.knn_plan(8192, 8192, 64) == 1  # a full batch needs none
    assert sift.Matcher.knn_plan(0, 0, 1, 1) == 1
    for bad in ((-1, 5, 1, 2), (5, -1, 1, 2), (5, 5, 0, 2)):
        assert L.sift_hip_match_knn_plan(*bad, ctypes.byref(S)) == INVALID
    assert L.sift_hip_match_knn_plan(5, 5, 1, 2, None) == INVALID
