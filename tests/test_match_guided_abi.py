"""Guided matching (sift_hip_match_guided_*, matchListGuided): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_match_gate has the layout
  of its ctypes mirror; the header still compiles as C99.
* A null matcher or gate, a radius that is not > 0 (0, negative, NaN) and a stride of 1 are SIFT_HIP_ERR_INVALID
  before any device call.
* The references the GPU tests hold the device to: sift_amd.cv.gate_mask on a hand-written case (the inclusive edge,
  a NaN row), and sift_amd.cv.guided_top2 without a gate against the CPU oracle's knn-2.
* The inputs of tests/test_gpu_match_guided.py (tests/guided_cases.py) do exercise the gate: queries with no, one and
  several candidates, a candidate on the window's edge, and a guided best that is mostly not the global best.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import guided_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
INVALID = -1  # SIFT_HIP_ERR_INVALID

NAMES = ("sift_hip_match_guided_device", "sift_hip_match_guided_plan", "sift_hip_match_list_guided_device",
         "sift_hip_match_list_guided_host")
SIGNATURES = """
#include "sift_hip.h"
int (*a)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_gate*, float, int, int*,
         float*, int*, void*) = sift_hip_match_guided_device;
int (*b)(int, int, int*) = sift_hip_match_guided_plan;
int (*c)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_gate*,
         const sift_hip_match_filter*, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_guided_device;
int (*d)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_gate*,
         const sift_hip_match_filter*, sift_hip_dmatch*, int, int*) = sift_hip_match_list_guided_host;
"""
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_match_gate), __builtin_offsetof(sift_hip_match_gate, query_xy),
                __builtin_offsetof(sift_hip_match_gate, query_stride), __builtin_offsetof(sift_hip_match_gate, train_xy),
                __builtin_offsetof(sift_hip_match_gate, train_stride), __builtin_offsetof(sift_hip_match_gate, radius)};
int main(void) {
    sift_hip_match_gate g = {0, 3, 0, 3, 1.0f};
    (void)g;
    for (int i = 0; i < 6; i++) printf("%d\\n", layout[i]);
    return 0;
}
"""


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
    assert len(L.sift_hip_match_guided_device.argtypes) == 12
    assert len(L.sift_hip_match_guided_plan.argtypes) == 3
    assert len(L.sift_hip_match_list_guided_device.argtypes) == 10
    assert len(L.sift_hip_match_list_guided_host.argtypes) == 10
    # the header as C99 (a function pointer of another type is an error), and the struct's layout from the C side
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    G = sift._MatchGate
    assert layout == [ctypes.sizeof(G), G.query_xy.offset, G.query_stride.offset, G.train_xy.offset,
                      G.train_stride.offset, G.radius.offset]


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv

    for name in ("match_guided_device", "match_list_guided_device", "match_list_guided_host", "guided_plan"):
        assert callable(getattr(sift.Matcher, name)), name
    params = inspect.signature(sift.matchListGuided).parameters
    assert list(params)[:7] == ["des", "num_des", "des_xy", "src", "num_src", "src_xy", "radius"]
    assert params["des_stride"].default == 3 and params["src_stride"].default == 3 and "filter" in params
    assert callable(cv.gate_mask) and callable(cv.guided_top2)
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::matchListGuided(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::MatchGate const&, " \
           "sift_cuda::MatchFilter const&)" in out
    assert "sift_cuda::matchGuided(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::MatchGate const&)" in out


def guided_calls(sift, m, gate):
    """Status and error text of the three entry points that take a gate, on host memory that must never be read."""
    L = sift.lib()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    f = sift._match_filter()
    n = ctypes.c_int(-7)
    g = ctypes.byref(gate) if gate is not None else None
    out = []
    for rc in (L.sift_hip_match_guided_device(m, p, 1, p, 1, g, 0.8, 0, p, p, p, None),
               L.sift_hip_match_list_guided_device(m, p, 1, p, 1, g, ctypes.byref(f), p, p, None),
               L.sift_hip_match_list_guided_host(m, p, 1, p, 1, g, ctypes.byref(f), p, 1, ctypes.byref(n))):
        out.append((rc, L.sift_hip_last_error().decode()))
    assert not buf.any()
    return out


def test_null_matcher_or_gate_is_invalid(sift):
    buf = np.zeros(8, np.float32)
    good = sift._MatchGate(buf.ctypes.data, 3, buf.ctypes.data, 3, 5.0)
    for rc, msg in guided_calls(sift, None, good):
        assert rc == INVALID and "matcher" in msg, msg
    fake = ctypes.c_void_p(buf.ctypes.data)  # the gate is looked at first: this matcher is never dereferenced
    for rc, msg in guided_calls(sift, fake, None):
        assert rc == INVALID and "gate" in msg, msg
    S = ctypes.c_int()
    assert sift.lib().sift_hip_match_guided_plan(10, 10, None) == INVALID
    assert sift.lib().sift_hip_match_guided_plan(-1, 10, ctypes.byref(S)) == INVALID


@pytest.mark.parametrize("radius", [0.0, -0.0, -3.0, float("nan"), -math.inf])
def test_bad_radius_is_refused(sift, radius):
    buf = np.zeros(8, np.float32)
    gate = sift._MatchGate(buf.ctypes.data, 3, buf.ctypes.data, 3, radius)
    for rc, msg in guided_calls(sift, None, gate):
        assert rc == INVALID and "radius" in msg, msg


@pytest.mark.parametrize("strides", [(1, 3), (3, 1), (0, 2), (-3, 3)])
def test_bad_stride_is_refused(sift, strides):
    buf = np.zeros(8, np.float32)
    gate = sift._MatchGate(buf.ctypes.data, strides[0], buf.ctypes.data, strides[1], 5.0)
    for rc, msg in guided_calls(sift, None, gate):
        assert rc == INVALID and "stride" in msg, msg


def test_guided_plan_host_only(sift):
    """One split per key group of 256 train rows while the launch stays under its workgroup target."""
    assert sift.Matcher.guided_plan(33, 31) == 1
    assert sift.Matcher.guided_plan(257, 300) == 2
    assert sift.Matcher.guided_plan(600, 1100) > 1
    assert sift.Matcher.guided_plan(0, 0) == 1


def test_gate_mask_hand_written(sift):
    from sift_amd import cv

    nan = np.nan
    q_xy = np.float32([[10, 10], [50, 50], [nan, 10]])
    t_xy = np.float32([[16, 4], [16.25, 10], [10, nan]])  # |dx| == |dy| == radius; just outside in x; a NaN row
    got = cv.gate_mask(q_xy, t_xy, 6.0)
    assert got.dtype == bool and got.shape == (3, 3)
    assert got.tolist() == [[True, False, False], [False, False, False], [False, False, False]]
    assert cv.gate_mask(q_xy, t_xy, np.inf).tolist() == [[True, True, False], [True, True, False], [False] * 3]
    # symmetric in the two rows, and further columns of a stride-3 array are ignored
    assert np.array_equal(cv.gate_mask(t_xy, q_xy, 6.0), got.T)
    assert np.array_equal(cv.gate_mask(gc.with_stride(q_xy, 3), gc.with_stride(t_xy, 3), 6.0), got)
    # float32 arithmetic: 2^24 + 1 is not a float32, so the difference to 2^24 is 0
    assert cv.gate_mask(np.float64([[2 ** 24 + 1, 0]]), np.float64([[2 ** 24, 0]]), 0.5).tolist() == [[True]]


@pytest.mark.parametrize("nq,nt", [(33, 31), (257, 300)])
def test_guided_top2_without_a_gate_is_the_oracle(sift, oracle, nq, nt):
    """radius = inf: the reference is the CPU oracle's knn-2 (distances sqrtf(s) of exact integer sums s < 2^22,
    recovered as rint(dist^2))."""
    from sift_amd import cv

    q, t, q_xy, t_xy = gc.make_guided(nq, nt)
    for a, b, axy, bxy in ((q, t, q_xy, t_xy), (t, q, t_xy, q_xy)):
        idx, dist = oracle.knn2(a, b)
        gi, gd = cv.guided_top2(a, b, axy, bxy, np.inf)
        assert gi.dtype == np.int32 and gd.dtype == np.float32 and gi.shape == gd.shape == (len(a), 2)
        assert np.array_equal(gi, idx)
        assert np.array_equal(gd, np.rint(dist.astype(np.float64) ** 2).astype(np.float32))


def test_guided_top2_small_cases(sift):
    from sift_amd import cv

    q = np.zeros((3, 128), np.float32)
    t = np.zeros((4, 128), np.float32)
    t[:, 0] = [3, 1, 1, 2]
    q_xy = np.float32([[0, 0], [100, 100], [0, 0]])
    t_xy = np.float32([[0, 0], [50, 50], [1, 1], [1, -1]])
    idx, d2 = cv.guided_top2(q, t, q_xy, t_xy, 2.0)
    # query 0: candidates 0, 2, 3 (row 1, the tie partner of row 2, is outside); query 1: none
    assert idx.tolist() == [[2, 3], [-1, -1], [2, 3]]
    assert d2.tolist() == [[1, 4], [gc.FLT_MAX, gc.FLT_MAX], [1, 4]]
    idx, d2 = cv.guided_top2(q, t, q_xy, t_xy, 60.0)  # the tie 1 / 2 goes to the lower index; query 1 sees row 1 only
    assert idx.tolist() == [[1, 2], [1, -1], [1, 2]] and d2[1].tolist() == [1, gc.FLT_MAX]
    for a, b in ((q[:0], t), (q, t[:0])):
        idx, d2 = cv.guided_top2(a, b, q_xy[:len(a)], t_xy[:len(b)], 2.0)
        assert idx.shape == (len(a), 2) and np.all(idx == -1) and np.all(d2 == gc.FLT_MAX)
    got = cv.filter_matches(*cv.guided_top2(q, t, q_xy, t_xy, 2.0), *cv.guided_top2(t, q, t_xy, q_xy, 2.0), ratio=0.0)
    assert got["queryIdx"].tolist() == [0] and got["trainIdx"].tolist() == [2]


def test_the_gpu_cases_exercise_the_gate(sift):
    from sift_amd import cv

    union = np.zeros(3, bool)
    edge = False
    for nq, nt in gc.SHAPES:
        q, t, q_xy, t_xy, (gi, gd), _ = gc.case(nq, nt)
        assert np.all(q_xy * 4 == np.rint(q_xy * 4)) and q_xy.min() >= 0 and q_xy.max() < gc.SIDE
        assert np.all(t_xy * 4 == np.rint(t_xy * 4)) and t_xy.min() >= 0 and t_xy.max() < gc.SIDE
        cand = cv.gate_mask(q_xy, t_xy, gc.RADIUS)
        ncand = cand.sum(1)
        assert np.array_equal(ncand >= 1, gi[:, 0] >= 0) and np.array_equal(ncand >= 2, gi[:, 1] >= 0)
        kinds = np.array([(ncand == 0).any(), (ncand == 1).any(), (ncand >= 2).any()])
        on_edge = bool((cand & (np.abs(t_xy[None, :, 0] - q_xy[:, None, 0]) == gc.RADIUS)).any())
        union |= kinds
        edge |= on_edge
        if nq >= 31 and nt >= 31:
            assert kinds.all() and on_edge, (nq, nt, kinds, on_edge)
            free, _ = cv.guided_top2(q, t, q_xy, t_xy, np.inf)
            has = gi[:, 0] >= 0
            assert (gi[has, 0] != free[has, 0]).mean() > 0.5, (nq, nt)  # a kernel that ignores the gate cannot pass
    assert union.all() and edge
