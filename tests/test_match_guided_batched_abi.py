"""Batched guided matching (sift_hip_match_*_guided_batched / *_epipolar_batched,
sift_hip_project_homography_batched_device): what runs without a GPU, after tests/test_match_guided_abi.py.

* The entry points are exported with the signatures include/sift_hip.h documents; the two record types have the layout
  of their ctypes mirrors; the header still compiles as C99 and no longer says the batched forms do not exist.
* Every rule of a gated call that needs no matcher -- a stride below 2, a radius that is not > 0, a max_error that is
  not > 0 and finite, a null geometry, a bad geometry stride -- is SIFT_HIP_ERR_INVALID with the documented message
  before the matcher is looked at, and a null matcher after them; the projection's own rules likewise.  None of the
  calls reads or writes the (host) memory it is handed.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
INVALID = -1  # SIFT_HIP_ERR_INVALID

NAMES = {"sift_hip_match_guided_batched": 16, "sift_hip_match_epipolar_batched": 19,
         "sift_hip_match_list_guided_batched": 14, "sift_hip_match_list_epipolar_batched": 17,
         "sift_hip_match_list_guided_codes_batched": 18, "sift_hip_match_list_epipolar_codes_batched": 21,
         "sift_hip_project_homography_batched_device": 7}
SIGNATURES = """
#include "sift_hip.h"
typedef const uint16_t* const* sets;
typedef const sift_hip_match_positions* pos;
typedef const sift_hip_match_filter* flt;
int (*a)(sift_hip_matcher_t, int, sets, const int*, sets, const int*, pos, int, int, float, float, int, int*, float*,
         int*, void*) = sift_hip_match_guided_batched;
int (*b)(sift_hip_matcher_t, int, sets, const int*, sets, const int*, pos, int, int, float, const void*, int, float,
         float, int, int*, float*, int*, void*) = sift_hip_match_epipolar_batched;
int (*c)(sift_hip_matcher_t, int, sets, const int*, sets, const int*, pos, int, int, float, flt, sift_hip_dmatch*, int*,
         void*) = sift_hip_match_list_guided_batched;
int (*d)(sift_hip_matcher_t, int, sets, const int*, sets, const int*, pos, int, int, float, const void*, int, float,
         flt, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_epipolar_batched;
int (*e)(sift_hip_matcher_t, const int8_t*, const int*, int, const int*, const int*, const int*, const int*, const int*,
         const int*, pos, int, int, float, flt, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_guided_codes_batched;
int (*f)(sift_hip_matcher_t, const int8_t*, const int*, int, const int*, const int*, const int*, const int*, const int*,
         const int*, pos, int, int, float, const void*, int, float, flt, sift_hip_dmatch*, int*,
         void*) = sift_hip_match_list_epipolar_codes_batched;
int (*g)(const void*, int, int, const sift_hip_project_set*, int, int, void*) = sift_hip_project_homography_batched_device;
int abi[SIFT_HIP_ABI_VERSION == 1 ? 1 : -1];
"""
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_match_positions), __builtin_offsetof(sift_hip_match_positions, query_xy),
                __builtin_offsetof(sift_hip_match_positions, train_xy), sizeof(sift_hip_project_set),
                __builtin_offsetof(sift_hip_project_set, xy), __builtin_offsetof(sift_hip_project_set, n),
                __builtin_offsetof(sift_hip_project_set, out_xy)};
int main(void) {
    for (int i = 0; i < 7; i++) printf("%d\\n", layout[i]);
    return 0;
}
"""


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name, nargs in NAMES.items():
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == nargs, name
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = sift._MatchPositions, sift._ProjectSet
    assert layout == [ctypes.sizeof(P), P.query_xy.offset, P.train_xy.offset, ctypes.sizeof(S), S.xy.offset, S.n.offset,
                      S.out_xy.offset]


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv, multi

    for name in ("match_guided_batched", "match_list_guided_batched", "match_epipolar_batched",
                 "match_list_epipolar_batched", "match_list_guided_codes_batched", "match_list_epipolar_codes_batched"):
        assert callable(getattr(sift.Matcher, name)), name
    assert inspect.signature(sift.Matcher.match_list_epipolar_batched).parameters["geometry_stride"].default == 52
    assert list(inspect.signature(sift.project_homography_batched_device).parameters)[:2] == ["geometry_ptr", "sets"]
    assert list(inspect.signature(sift.matchListGuidedBatched).parameters)[:3] == ["desc_per_pair", "xy_per_pair", "radius"]
    assert list(inspect.signature(sift.matchListEpipolarBatched).parameters)[:4] == ["desc_per_pair", "xy_per_pair",
                                                                                     "F_per_pair", "max_error"]
    assert callable(cv.geometry_usable) and "guided" in multi.position_pairs.__doc__
    header = open(os.path.join(ROOT, "include", "sift_hip.h")).read()
    assert "guided forms do not exist" not in " ".join(header.split())
    assert "sift_hip_match_list_epipolar_batched" in header and "geometry_usable" in header
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    for name in ("sift_cuda::matchListGuidedBatchedDevice(sift_cuda::BatchMatcher&",
                 "sift_cuda::matchListEpipolarBatchedDevice(sift_cuda::BatchMatcher&",
                 "sift_cuda::projectHomographyBatchedDevice(void const*, int"):
        assert name in out, name


def gated_calls(sift, m, epipolar, qs=2, ts=2, radius=5.0, geometry="buf", gstride=36, max_error=1.5):
    """Status and error text of the three entry points of a gate, on host memory that must never be read or written."""
    L = sift.lib()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    f = sift._match_filter()
    pos = (sift._MatchPositions * 1)(sift._MatchPositions(p, p))
    g = p if geometry == "buf" else geometry
    if epipolar:
        rcs = (L.sift_hip_match_epipolar_batched(m, 1, p, p, p, p, pos, qs, ts, radius, g, gstride, max_error, 0.8, 0, p,
                                                 p, p, None),
               L.sift_hip_match_list_epipolar_batched, L.sift_hip_match_list_epipolar_codes_batched)
    else:
        rcs = (L.sift_hip_match_guided_batched(m, 1, p, p, p, p, pos, qs, ts, radius, 0.8, 0, p, p, p, None),
               L.sift_hip_match_list_guided_batched, L.sift_hip_match_list_guided_codes_batched)
    out = [(rcs[0], L.sift_hip_last_error().decode())]
    tail = (g, gstride, max_error) if epipolar else ()
    rc = rcs[1](m, 1, p, p, p, p, pos, qs, ts, radius, *tail, ctypes.byref(f), p, p, None)
    out.append((rc, L.sift_hip_last_error().decode()))
    rc = rcs[2](m, p, p, 1, p, p, p, p, p, p, pos, qs, ts, radius, *tail, ctypes.byref(f), p, p, None)
    out.append((rc, L.sift_hip_last_error().decode()))
    assert not buf.any()
    return out


@pytest.mark.parametrize("epipolar", [False, True])
def test_null_matcher_is_invalid(sift, epipolar):
    for rc, msg in gated_calls(sift, None, epipolar):
        assert rc == INVALID and msg == "null matcher", msg


@pytest.mark.parametrize("epipolar", [False, True])
@pytest.mark.parametrize("radius", [0.0, -0.0, -3.0, float("nan"), -math.inf])
def test_bad_radius_is_refused(sift, epipolar, radius):
    gate = "epipolar gate" if epipolar else "match gate"
    for rc, msg in gated_calls(sift, None, epipolar, radius=radius):
        assert rc == INVALID and msg == gate + ": the radius must be > 0", msg


@pytest.mark.parametrize("epipolar", [False, True])
@pytest.mark.parametrize("strides", [(1, 3), (3, 1), (0, 2), (-3, 3)])
def test_bad_stride_is_refused(sift, epipolar, strides):
    gate = "epipolar gate" if epipolar else "match gate"
    for rc, msg in gated_calls(sift, None, epipolar, qs=strides[0], ts=strides[1]):
        assert rc == INVALID and msg == gate + ": a position stride below 2 floats", msg


@pytest.mark.parametrize("max_error", [0.0, -1.0, float("nan"), math.inf])
def test_bad_max_error_is_refused(sift, max_error):
    for rc, msg in gated_calls(sift, None, True, max_error=max_error):
        assert rc == INVALID and msg == "epipolar gate: max_error must be > 0 and finite", msg


def test_bad_geometry_is_refused(sift):
    """The gate's own rules come before the matcher: the fake matcher below is never dereferenced."""
    fake = ctypes.c_void_p(np.zeros(8, np.float32).ctypes.data)
    for m in (None, fake):
        for rc, msg in gated_calls(sift, m, True, geometry=None):
            assert rc == INVALID and msg == "epipolar gate: null geometry", msg
        for gstride in (0, 32, 35, 38, 50, -52):
            for rc, msg in gated_calls(sift, m, True, gstride=gstride):
                assert rc == INVALID and msg == "epipolar gate: geometry_stride_bytes must be >= 36 and a multiple of 4", msg
    for gstride in (36, 40, 52, 4096):  # good strides reach the matcher check
        for rc, msg in gated_calls(sift, None, True, gstride=gstride):
            assert rc == INVALID and msg == "null matcher", msg


def project(sift, geometry="buf", gstride=36, P=1, sets="one", stride=2, out_stride=2, n=4, xy=0, out=256):
    L = sift.lib()
    buf = np.zeros(256, np.float32)
    p = buf.ctypes.data
    table = None
    if sets == "one":
        table = (sift._ProjectSet * max(P, 1))(*[sift._ProjectSet(None if xy is None else p + xy, n,
                                                                   None if out is None else p + out)] * max(P, 1))
    rc = L.sift_hip_project_homography_batched_device(p + 512 if geometry == "buf" else geometry, gstride, P, table,
                                                      stride, out_stride, None)
    assert not buf.any()
    return rc, L.sift_hip_last_error().decode()


def test_projection_rules(sift):
    for kw, msg in ((dict(geometry=None), "project: null geometry"),
                    (dict(gstride=32), "project: geometry_stride_bytes must be >= 36 and a multiple of 4"),
                    (dict(gstride=54), "project: geometry_stride_bytes must be >= 36 and a multiple of 4"),
                    (dict(P=0), "project: bad batch"), (dict(P=65), "project: bad batch"),
                    (dict(sets=None), "project: bad batch"),
                    (dict(stride=1), "project: a position stride below 2 floats"),
                    (dict(out_stride=1), "project: a position stride below 2 floats"),
                    (dict(n=-1), "project: a negative row count"),
                    (dict(xy=None), "project: null position pointer"),
                    (dict(out=None), "project: null position pointer"),
                    (dict(out=8), "project: out_xy overlaps xy (only out_xy == xy with equal strides may)"),
                    (dict(out=0, out_stride=3), "project: out_xy overlaps xy (only out_xy == xy with equal strides may)")):
        rc, got = project(sift, **kw)
        assert rc == INVALID and got == msg, (kw, got)
    # all sets empty: nothing to launch, no device needed
    assert project(sift, n=0, xy=None, out=None)[0] == 0
    assert project(sift, P=3, n=0)[0] == 0
