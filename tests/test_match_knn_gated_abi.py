"""Gated k nearest neighbours (sift_hip_match_knn_guided_* / *_epipolar_*): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents; the Python and C++ surfaces exist.
* Every refusal that needs no matcher -- k outside 1..SIFT_HIP_KNN_MAX, a NaN max_distance, a stride < 2, a radius not
  > 0, a max_error not > 0 or not finite, an unusable host F, a null geometry, a geometry stride < 36 or not a
  multiple of 4 -- returns SIFT_HIP_ERR_INVALID with a message naming the cause and no byte written, before the
  matcher is looked at (the handle passed here is never dereferenced).  Then a null gate and a null matcher.  The
  refusals that need a matcher's limits are in tests/test_gpu_match_knn_gated.py.
* The header no longer says gated k-NN is missing; it does say the _codes_batched gated k-NN forms are.
"""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")

SIGNATURES = """
#include "sift_hip.h"
_Static_assert(SIFT_HIP_KNN_MAX == 8, "two kernel instantiations per gate: 4 and 8 entries");
_Static_assert(SIFT_HIP_ABI_VERSION == 1, "additions only");
#define SETS const uint16_t*, int, const uint16_t*, int
#define BATCH int, const uint16_t* const*, const int*, const uint16_t* const*, const int*, const sift_hip_match_positions*, int, int, float
int (*a)(sift_hip_matcher_t, SETS, const sift_hip_match_gate*, int, int*, float*, void*) = sift_hip_match_knn_guided_device;
int (*b)(sift_hip_matcher_t, SETS, const sift_hip_match_epipolar_gate*, int, int*, float*, void*) =
    sift_hip_match_knn_epipolar_device;
int (*c)(sift_hip_matcher_t, BATCH, int, int*, float*, void*) = sift_hip_match_knn_guided_batched;
int (*d)(sift_hip_matcher_t, BATCH, const void*, int, float, int, int*, float*, void*) = sift_hip_match_knn_epipolar_batched;
int (*e)(sift_hip_matcher_t, SETS, const sift_hip_match_gate*, int, float, sift_hip_dmatch*, int*, void*) =
    sift_hip_match_knn_list_guided_device;
int (*f)(sift_hip_matcher_t, SETS, const sift_hip_match_epipolar_gate*, int, float, sift_hip_dmatch*, int*, void*) =
    sift_hip_match_knn_list_epipolar_device;
int (*g)(sift_hip_matcher_t, BATCH, int, float, sift_hip_dmatch*, int*, void*) = sift_hip_match_knn_list_guided_batched;
int (*h)(sift_hip_matcher_t, BATCH, const void*, int, float, int, float, sift_hip_dmatch*, int*, void*) =
    sift_hip_match_knn_list_epipolar_batched;
int (*i)(sift_hip_matcher_t, SETS, const sift_hip_match_gate*, int, int*, float*) = sift_hip_match_knn_guided_host;
int (*j)(sift_hip_matcher_t, SETS, const sift_hip_match_epipolar_gate*, int, int*, float*) = sift_hip_match_knn_epipolar_host;
int (*k)(sift_hip_matcher_t, SETS, const sift_hip_match_gate*, int, float, sift_hip_dmatch*, int, int*) =
    sift_hip_match_knn_list_guided_host;
int (*l)(sift_hip_matcher_t, SETS, const sift_hip_match_epipolar_gate*, int, float, sift_hip_dmatch*, int, int*) =
    sift_hip_match_knn_list_epipolar_host;
"""
NAMES = {"sift_hip_match_knn_guided_device": 10, "sift_hip_match_knn_epipolar_device": 10,
         "sift_hip_match_knn_guided_batched": 14, "sift_hip_match_knn_epipolar_batched": 17,
         "sift_hip_match_knn_list_guided_device": 11, "sift_hip_match_knn_list_epipolar_device": 11,
         "sift_hip_match_knn_list_guided_batched": 15, "sift_hip_match_knn_list_epipolar_batched": 18,
         "sift_hip_match_knn_guided_host": 9, "sift_hip_match_knn_epipolar_host": 9,
         "sift_hip_match_knn_list_guided_host": 11, "sift_hip_match_knn_list_epipolar_host": 11}
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

    for name in ("match_knn_guided_device", "match_knn_epipolar_device", "match_knn_guided_batched",
                 "match_knn_epipolar_batched", "match_knn_list_guided_device", "match_knn_list_epipolar_device",
                 "match_knn_list_guided_batched", "match_knn_list_epipolar_batched", "match_knn_guided_host",
                 "match_knn_epipolar_host", "match_knn_list_guided_host", "match_knn_list_epipolar_host"):
        assert callable(getattr(sift.Matcher, name)), name
    sets = ["des", "num_des", "des_xy", "src", "num_src", "src_xy"]
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(sift.knnMatchGuided)[:8] == sets + ["radius", "k"]
    assert par(sift.knnMatchEpipolar)[:10] == sets + ["F", "max_error", "k", "radius"]
    assert par(sift.matchKnnListGuided)[:9] == sets + ["radius", "k", "max_distance"]
    assert par(sift.matchKnnListEpipolar)[:10] == sets + ["F", "max_error", "k", "max_distance"]
    assert par(cv.mask_knn) == ["q", "t", "cand", "k"]
    assert par(cv.guided_knn) == ["q", "t", "q_xy", "t_xy", "radius", "k"]
    assert par(cv.epipolar_knn) == ["q", "t", "q_xy", "t_xy", "F", "max_error", "k", "radius"]
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    half = "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, "
    assert f"sift_cuda::matchKnnGuided({half}sift_cuda::MatchGate const&, int)" in out
    assert f"sift_cuda::matchKnnEpipolar({half}sift_cuda::EpipolarGate const&, int)" in out
    assert f"sift_cuda::matchKnnListGuided({half}sift_cuda::MatchGate const&, int, float)" in out
    assert f"sift_cuda::matchKnnListEpipolar({half}sift_cuda::EpipolarGate const&, int, float)" in out
    for name in ("matchKnnGuidedBatchedDevice", "matchKnnEpipolarBatchedDevice", "matchKnnListGuidedBatchedDevice",
                 "matchKnnListEpipolarBatchedDevice"):
        assert f"sift_cuda::{name}(sift_cuda::BatchMatcher&" in out, name


def test_documents(sift):
    for doc in ("include/sift_hip.h", "README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, doc)).read().replace("*", " ").split())
        assert "of k-NN are not provided" not in text and "epipolar) k-NN is not provided" not in text, doc
        assert "_codes_batched" in text and "sift_hip_match_knn_guided_device" in text, doc
    header = " ".join(open(os.path.join(ROOT, "include", "sift_hip.h")).read().replace("*", " ").split())
    assert "Gated k-NN on ready code sets (_codes_batched) is not provided" in header


def test_refusals_that_need_no_matcher(sift):
    L = sift.lib()
    buf = np.full(64, -7, np.int32)
    p = buf.ctypes.data
    pp = ctypes.c_void_p(p)
    one = ctypes.c_int(1)
    n = ctypes.c_int(-7)
    fake = ctypes.c_void_p(p)  # never dereferenced: these rules are judged before the matcher is looked at
    F = np.float32([[0, -1, 450], [1, 0, 700], [-450, -700, 0]])
    inf, nan = float("inf"), float("nan")
    pos = sift._MatchPositions(p, p)
    P = ctypes.byref(pos)

    def refused(rc, word):
        msg = L.sift_hip_last_error().decode()
        assert rc == INVALID and word in msg, (rc, msg, word)

    def window(qs=2, ts=2, radius=5.0):
        return ctypes.byref(sift._MatchGate(p, qs, p, ts, radius))

    def band(qs=2, ts=2, radius=inf, F=F, max_error=2.0):
        return ctypes.byref(sift._epipolar_gate(p, qs, p, ts, radius, F, max_error))

    sets = (p, 1, p, 1)
    bsets = (1, ctypes.byref(pp), ctypes.byref(one), ctypes.byref(pp), ctypes.byref(one), P)

    def calls(k=2, md=0.0, w=None, b=None, strides=(2, 2), radius=5.0, geo=p, gstride=36, max_error=2.0, matcher=fake):
        """Every entry point by a short name (w_: window, e_: epipolar), with one argument made bad."""
        w, b = w or window(), b or band()
        return {
            "w_dev": lambda: L.sift_hip_match_knn_guided_device(matcher, *sets, w, k, p, p, None),
            "w_host": lambda: L.sift_hip_match_knn_guided_host(matcher, *sets, w, k, p, p),
            "w_list": lambda: L.sift_hip_match_knn_list_guided_device(matcher, *sets, w, k, md, p, p, None),
            "w_list_host": lambda: L.sift_hip_match_knn_list_guided_host(matcher, *sets, w, k, md, p, 1, ctypes.byref(n)),
            "w_batch": lambda: L.sift_hip_match_knn_guided_batched(matcher, *bsets, *strides, radius, k, p, p, None),
            "w_list_batch": lambda: L.sift_hip_match_knn_list_guided_batched(matcher, *bsets, *strides, radius, k, md, p,
                                                                             p, None),
            "e_dev": lambda: L.sift_hip_match_knn_epipolar_device(matcher, *sets, b, k, p, p, None),
            "e_host": lambda: L.sift_hip_match_knn_epipolar_host(matcher, *sets, b, k, p, p),
            "e_list": lambda: L.sift_hip_match_knn_list_epipolar_device(matcher, *sets, b, k, md, p, p, None),
            "e_list_host": lambda: L.sift_hip_match_knn_list_epipolar_host(matcher, *sets, b, k, md, p, 1,
                                                                           ctypes.byref(n)),
            "e_batch": lambda: L.sift_hip_match_knn_epipolar_batched(matcher, *bsets, *strides, radius, geo, gstride,
                                                                     max_error, k, p, p, None),
            "e_list_batch": lambda: L.sift_hip_match_knn_list_epipolar_batched(matcher, *bsets, *strides, radius, geo,
                                                                               gstride, max_error, k, md, p, p, None),
        }

    def all_refused(word, only=None, **kw):
        """Every entry point the defect applies to (`only`) refuses, with a message naming the cause."""
        hit = 0
        for name, call in calls(**kw).items():
            if only is None or only(name):
                refused(call(), word)
                hit += 1
        assert hit

    is_list = lambda name: "list" in name  # noqa: E731
    is_batch = lambda name: "batch" in name  # noqa: E731
    is_epi = lambda name: name.startswith("e_")  # noqa: E731
    for k in (0, -1, 9):
        all_refused("k outside", k=k)
    all_refused("NaN", only=is_list, md=nan)
    # k is judged before max_distance, both before the gate
    all_refused("k outside", k=9, md=nan, w=window(qs=1), b=band(qs=1), strides=(1, 2))
    all_refused("NaN", only=is_list, md=nan, w=window(radius=0.0), b=band(max_error=0.0), radius=0.0, max_error=0.0)
    for qs, ts in ((1, 2), (2, 1), (0, 0)):
        all_refused("stride", w=window(qs, ts), b=band(qs, ts), strides=(qs, ts))
    for r in (0.0, -1.0, nan):
        all_refused("radius", w=window(radius=r), b=band(radius=r), radius=r)
    for e in (0.0, -2.0, inf, nan):
        all_refused("max_error", only=is_epi, b=band(max_error=e), max_error=e)
    bad_F = F.copy()
    bad_F[2, 1] = nan
    all_refused("non-finite", only=lambda x: is_epi(x) and not is_batch(x), b=band(F=bad_F))
    all_refused("all zero", only=lambda x: is_epi(x) and not is_batch(x), b=band(F=np.zeros(9, np.float32)))
    all_refused("null geometry", only=lambda x: is_epi(x) and is_batch(x), geo=None)
    for gs in (35, 32, 38, 0, -36):
        all_refused("geometry_stride", only=lambda x: is_epi(x) and is_batch(x), gstride=gs)
    # then a null gate and a null matcher
    for name, rc in [("w", L.sift_hip_match_knn_guided_device(fake, *sets, None, 2, p, p, None)),
                     ("e", L.sift_hip_match_knn_epipolar_device(fake, *sets, None, 2, p, p, None)),
                     ("wl", L.sift_hip_match_knn_list_guided_device(fake, *sets, None, 2, 0.0, p, p, None)),
                     ("eh", L.sift_hip_match_knn_epipolar_host(fake, *sets, None, 2, p, p))]:
        assert rc == INVALID and "gate" in L.sift_hip_last_error().decode(), name
    all_refused("null matcher", matcher=None)
    refused(L.sift_hip_match_knn_list_guided_host(None, *sets, window(), 2, 0.0, p, 1, None), "null out or count")
    assert n.value == 0  # the host lists' count is cleared, nothing else is written
    assert (buf == -7).all()
