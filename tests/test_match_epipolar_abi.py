"""The epipolar gate (sift_hip_match_epipolar_*, matchListEpipolar): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents; sift_hip_match_epipolar_gate has the
  layout of its ctypes mirror; the header still compiles as C99.
* Every argument the header lists as invalid that can be judged without a matcher (a null matcher or gate, the
  strides, the radius, max_error, F) is SIFT_HIP_ERR_INVALID before any device call, with a message that names it, on
  host memory that is never read; sizes over a matcher's limits and null pointers of non-empty sets need a matcher and
  are in tests/test_gpu_match_epipolar.py.
* The references the GPU tests hold the device to: sift_amd.cv.epipolar_mask on the hand-written case (the inclusive
  edge, a NaN row, further columns ignored, the window ANDed with the band), and sift_amd.cv.epipolar_top2 with every
  row a candidate against the CPU oracle's knn-2.
* The inputs of tests/test_gpu_match_epipolar.py (tests/epipolar_cases.py) do exercise the gate: queries with no, one
  and several candidates, a candidate on the band's edge, every planted pair inside the band, and a guided best that
  is mostly not the global best.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import epipolar_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")
INVALID = -1  # SIFT_HIP_ERR_INVALID

NAMES = ("sift_hip_match_epipolar_device", "sift_hip_match_list_epipolar_device", "sift_hip_match_list_epipolar_host")
SIGNATURES = """
#include "sift_hip.h"
int (*a)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_epipolar_gate*, float,
         int, int*, float*, int*, void*) = sift_hip_match_epipolar_device;
int (*c)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_epipolar_gate*,
         const sift_hip_match_filter*, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_epipolar_device;
int (*d)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_epipolar_gate*,
         const sift_hip_match_filter*, sift_hip_dmatch*, int, int*) = sift_hip_match_list_epipolar_host;
"""
FIELDS = ("query_xy", "query_stride", "train_xy", "train_stride", "radius", "F", "max_error")
LAYOUT = """
#include <stdio.h>
#include "sift_hip.h"
int layout[] = {sizeof(sift_hip_match_epipolar_gate), sizeof(((sift_hip_match_epipolar_gate*)0)->F), %s};
int main(void) {
    sift_hip_match_epipolar_gate g = {0, 3, 0, 3, 1.0f, {0, 0, 0, 0, 0, 0, 0, 0, 1}, 1.5f};
    (void)g;
    for (unsigned i = 0; i < sizeof layout / sizeof *layout; i++) printf("%%d\\n", layout[i]);
    return 0;
}
""" % ", ".join(f"__builtin_offsetof(sift_hip_match_epipolar_gate, {f})" for f in FIELDS)

GOOD_F = [0, 0, 0.5, 0, 0, -1, 0, 1, 0]


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    L = sift.lib()
    for name in NAMES:
        assert name in exported, name
    assert len(L.sift_hip_match_epipolar_device.argtypes) == 12
    assert len(L.sift_hip_match_list_epipolar_device.argtypes) == 10
    assert len(L.sift_hip_match_list_epipolar_host.argtypes) == 10
    assert "abi=1" in sift.version()
    sig, src, exe = tmp_path / "signatures.c", tmp_path / "layout.c", tmp_path / "layout"
    sig.write_text(SIGNATURES)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(sig)],
                   check=True)
    src.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    layout = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    G = sift._MatchEpipolarGate
    assert layout == [ctypes.sizeof(G), ctypes.sizeof(ctypes.c_float * 9)] + [getattr(G, f).offset for f in FIELDS]


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv

    for name in ("match_epipolar_device", "match_list_epipolar_device", "match_list_epipolar_host"):
        assert callable(getattr(sift.Matcher, name)), name
    params = inspect.signature(sift.matchListEpipolar).parameters
    assert list(params)[:8] == ["des", "num_des", "des_xy", "src", "num_src", "src_xy", "F", "max_error"]
    assert params["radius"].default == math.inf
    assert params["des_stride"].default == 3 and params["src_stride"].default == 3 and "filter" in params
    assert callable(cv.epipolar_mask) and callable(cv.epipolar_top2)
    assert list(inspect.signature(cv.guided_top2).parameters) == ["q", "t", "q_xy", "t_xy", "radius"]
    assert inspect.signature(cv.epipolar_mask).parameters["radius"].default == math.inf
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::matchListEpipolar(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::EpipolarGate const&, " \
           "sift_cuda::MatchFilter const&)" in out
    assert "sift_cuda::matchEpipolar(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::EpipolarGate const&)" in out


def gate(sift, buf, qs=3, ts=3, radius=math.inf, F=GOOD_F, max_error=1.5, qxy=True, txy=True):
    p = buf.ctypes.data
    return sift._MatchEpipolarGate(p if qxy else None, qs, p if txy else None, ts, radius, (ctypes.c_float * 9)(*F),
                                   max_error)


def epipolar_calls(sift, m, g, nq=1, nt=1, q=True, t=True):
    """Status and error text of the three entry points that take the gate, on host memory that must never be read."""
    L = sift.lib()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    f = sift._match_filter()
    n = ctypes.c_int(-7)
    gp = ctypes.byref(g) if g is not None else None
    qp, tp = (p if q else None), (p if t else None)
    out = []
    for rc in (L.sift_hip_match_epipolar_device(m, qp, nq, tp, nt, gp, 0.8, 0, p, p, p, None),
               L.sift_hip_match_list_epipolar_device(m, qp, nq, tp, nt, gp, ctypes.byref(f), p, p, None),
               L.sift_hip_match_list_epipolar_host(m, qp, nq, tp, nt, gp, ctypes.byref(f), p, 1, ctypes.byref(n))):
        out.append((rc, L.sift_hip_last_error().decode()))
    assert not buf.any()
    return out


def test_null_matcher_or_gate_is_invalid(sift):
    buf = np.zeros(8, np.float32)
    for rc, msg in epipolar_calls(sift, None, gate(sift, buf)):
        assert rc == INVALID and "matcher" in msg, msg
    fake = ctypes.c_void_p(buf.ctypes.data)  # the gate is looked at first: this matcher is never dereferenced
    for rc, msg in epipolar_calls(sift, fake, None):
        assert rc == INVALID and "gate" in msg, msg


@pytest.mark.parametrize("radius", [0.0, -0.0, -3.0, float("nan"), -math.inf])
def test_bad_radius_is_refused(sift, radius):
    buf = np.zeros(8, np.float32)
    for rc, msg in epipolar_calls(sift, None, gate(sift, buf, radius=radius)):
        assert rc == INVALID and "radius" in msg, msg


@pytest.mark.parametrize("strides", [(1, 3), (3, 1), (0, 2), (-3, 3)])
def test_bad_stride_is_refused(sift, strides):
    buf = np.zeros(8, np.float32)
    for rc, msg in epipolar_calls(sift, None, gate(sift, buf, qs=strides[0], ts=strides[1])):
        assert rc == INVALID and "stride" in msg, msg


@pytest.mark.parametrize("max_error", [0.0, -0.0, -1.5, float("nan"), math.inf, -math.inf])
def test_bad_max_error_is_refused(sift, max_error):
    buf = np.zeros(8, np.float32)
    for rc, msg in epipolar_calls(sift, None, gate(sift, buf, max_error=max_error)):
        assert rc == INVALID and "max_error" in msg, msg


@pytest.mark.parametrize("k,v", [(0, math.nan), (4, math.inf), (8, -math.inf), (None, 0.0)])
def test_bad_F_is_refused(sift, k, v):
    buf = np.zeros(8, np.float32)
    F = [0.0] * 9 if k is None else [v if i == k else x for i, x in enumerate(GOOD_F)]
    for rc, msg in epipolar_calls(sift, None, gate(sift, buf, F=F)):
        assert rc == INVALID and "F" in msg and ("zero" in msg if k is None else "finite" in msg), msg


def test_epipolar_mask_hand_written(sift):
    from sift_amd import cv

    h = ec.HAND
    got = cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], h["max_error"])
    assert got.dtype == bool and got.shape == (1, 3) and got.tolist() == h["mask"]
    # the edge is exact: r r == e2 (nq + nr) == 9 for train (4, 1)
    F = h["F"].reshape(-1)
    qx, qy = h["q_xy"][0]
    a, b, c = (F[0] * qx + F[1] * qy) + F[2], (F[3] * qx + F[4] * qy) + F[5], (F[6] * qx + F[7] * qy) + F[8]
    tx, ty = h["t_xy"][0]
    u, v = (F[0] * tx + F[3] * ty) + F[6], (F[1] * tx + F[4] * ty) + F[7]
    r = (a * tx + b * ty) + c
    e2 = np.float32(h["max_error"]) * np.float32(h["max_error"])
    assert r * r == 9 and e2 * ((a * a + b * b) + (u * u + v * v)) == 9
    # F as 9 floats or 3 x 3; the reverse direction is F transposed with the roles swapped
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], F.tolist(), h["max_error"]).tolist() == h["mask"]
    assert cv.epipolar_mask(h["t_xy"], h["q_xy"], h["F"].T, h["max_error"]).tolist() == [[True], [False], [True]]
    # a NaN row is a candidate of nothing, on either side
    nan = np.nan
    t_nan = np.float32([[4, 1], [nan, 1], [3.75, nan]])
    assert cv.epipolar_mask(h["q_xy"], t_nan, h["F"], h["max_error"]).tolist() == [[True, False, False]]
    assert not cv.epipolar_mask(np.float32([[nan, 2]]), h["t_xy"], h["F"], h["max_error"]).any()
    assert not cv.epipolar_mask(np.float32([[7, nan]]), h["t_xy"], h["F"], 1e30).any()
    # further columns of a stride-3 array are ignored
    assert cv.epipolar_mask(ec.with_stride(h["q_xy"], 3), ec.with_stride(h["t_xy"], 5), h["F"],
                            h["max_error"]).tolist() == h["mask"]
    # the window is ANDed with the band: |dx| = 3, 2.75 and 3.25, |dy| = 1
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], h["max_error"], 3.0).tolist() == [[True, False, False]]
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], h["max_error"], 3.25).tolist() == h["mask"]
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], h["max_error"], 0.5).tolist() == [[False] * 3]
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], 1e30, 3.0).tolist() == [[True, True, False]]  # the window alone
    # float32 throughout: overflow is part of the rule (r r = inf <= inf), not an error
    big = np.float32([[3e38, 0]])
    with np.errstate(all="raise"):
        assert cv.epipolar_mask(big, big, np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1]), 1.0).shape == (1, 1)


@pytest.mark.parametrize("nq,nt", [(33, 31), (257, 300)])
def test_epipolar_top2_with_every_row_a_candidate_is_the_oracle(sift, oracle, nq, nt):
    """max_error = 1e30, radius = inf: the reference is the CPU oracle's knn-2 (distances sqrtf(s) of exact integer
    sums s < 2^22, recovered as rint(dist^2))."""
    from sift_amd import cv

    q, t, q_xy, t_xy, F, _, _, _ = ec.case(nq, nt)
    for a, b, axy, bxy, f in ((q, t, q_xy, t_xy, F), (t, q, t_xy, q_xy, F.T)):
        assert cv.epipolar_mask(axy, bxy, f, 1e30).all()
        idx, dist = oracle.knn2(a, b)
        gi, gd = cv.epipolar_top2(a, b, axy, bxy, f, 1e30, np.inf)
        assert gi.dtype == np.int32 and gd.dtype == np.float32 and gi.shape == gd.shape == (len(a), 2)
        assert np.array_equal(gi, idx)
        assert np.array_equal(gd, np.rint(dist.astype(np.float64) ** 2).astype(np.float32))


def test_guided_top2_is_unchanged_by_the_factoring(sift):
    """guided_top2 is mask_top2 of gate_mask: the small case of tests/test_match_guided_abi.py through both."""
    from sift_amd import cv

    q = np.zeros((3, 128), np.float32)
    t = np.zeros((4, 128), np.float32)
    t[:, 0] = [3, 1, 1, 2]
    q_xy = np.float32([[0, 0], [100, 100], [0, 0]])
    t_xy = np.float32([[0, 0], [50, 50], [1, 1], [1, -1]])
    idx, d2 = cv.guided_top2(q, t, q_xy, t_xy, 2.0)
    assert idx.tolist() == [[2, 3], [-1, -1], [2, 3]] and d2.tolist() == [[1, 4], [ec.FLT_MAX] * 2, [1, 4]]
    mi, md = cv.mask_top2(q, t, cv.gate_mask(q_xy, t_xy, 2.0))
    assert np.array_equal(mi, idx) and np.array_equal(md, d2)
    with pytest.raises(ValueError):
        cv.mask_top2(q, t, np.ones((3, 3), bool))


def test_the_gpu_cases_exercise_the_gate(sift):
    from sift_amd import cv

    h = ec.HAND
    assert cv.epipolar_mask(h["q_xy"], h["t_xy"], h["F"], h["max_error"]).tolist() == h["mask"]  # a candidate on the edge
    union = np.zeros(3, bool)
    for nq, nt in ec.SHAPES:
        q, t, q_xy, t_xy, F, (gi, gd), (ri, _), planted = ec.case(nq, nt)
        assert np.all(q_xy * 4 == np.rint(q_xy * 4)) and q_xy.min() >= 0 and q_xy.max() < ec.SIDE
        assert np.all(t_xy * 4 == np.rint(t_xy * 4)) and t_xy.min() >= 0 and t_xy.max() < ec.SIDE
        cand = cv.epipolar_mask(q_xy, t_xy, F, ec.MAX_ERROR)
        assert cand[planted[:, 0], planted[:, 1]].all()  # every true correspondence is inside the band
        assert cv.epipolar_mask(t_xy, q_xy, F.T, ec.MAX_ERROR)[planted[:, 1], planted[:, 0]].all()
        ncand = cand.sum(1)
        assert np.array_equal(ncand >= 1, gi[:, 0] >= 0) and np.array_equal(ncand >= 2, gi[:, 1] >= 0)
        kinds = np.array([(ncand == 0).any(), (ncand == 1).any(), (ncand >= 2).any()])
        union |= kinds
        if nq >= 31 and nt >= 31:
            assert kinds.all(), (nq, nt, kinds)
            free, _ = cv.epipolar_top2(q, t, q_xy, t_xy, F, 1e30)
            has = gi[:, 0] >= 0
            assert (gi[has, 0] != free[has, 0]).mean() > 0.5, (nq, nt)  # a kernel that ignores F cannot pass
            assert (gi[planted[:, 0], 0] == planted[:, 1]).mean() > 0.8  # the gate recovers the true correspondence
    assert union.all()
