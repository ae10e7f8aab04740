"""Match lists (sift_hip_match_list_*, matchList): what runs without a GPU.

* The entry points are exported with the signatures include/sift_hip.h documents; the record is 16 bytes.
* A null matcher is SIFT_HIP_ERR_INVALID.
* sift_amd.cv.filter_matches -- the reference the GPU tests hold the device operation to -- equals a brute-force
  O(nq nt) statement of the rule on tiny hand-made sets: duplicate rows in both sets (the tie rules of both
  directions), nt == 1, the empty set, and a non-mutual triangle.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "another-cuda-sift_amd", "lib")

SIGNATURES = """
#include "sift_hip.h"
_Static_assert(sizeof(sift_hip_dmatch) == 16, "cv::DMatch layout");
_Static_assert(sizeof(sift_hip_match_filter) == 20, "five 4-byte fields");
void (*d)(sift_hip_match_filter*) = sift_hip_default_match_filter;
int (*a)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_filter*, sift_hip_dmatch*,
         int*, void*) = sift_hip_match_list_device;
int (*b)(sift_hip_matcher_t, int, const uint16_t* const*, const int*, const uint16_t* const*, const int*,
         const sift_hip_match_filter*, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_batched;
int (*c)(sift_hip_matcher_t, const int8_t*, const int*, int, const int*, const int*, const int*, const int*, const int*,
         const int*, const sift_hip_match_filter*, sift_hip_dmatch*, int*, void*) = sift_hip_match_list_codes_batched;
int (*e)(sift_hip_matcher_t, const uint16_t*, int, const uint16_t*, int, const sift_hip_match_filter*, sift_hip_dmatch*,
         int, int*) = sift_hip_match_list_host;
int offsets[] = {__builtin_offsetof(sift_hip_dmatch, queryIdx), __builtin_offsetof(sift_hip_dmatch, trainIdx),
                 __builtin_offsetof(sift_hip_dmatch, imgIdx), __builtin_offsetof(sift_hip_dmatch, distance)};
"""
NAMES = ("sift_hip_match_list_device", "sift_hip_match_list_batched", "sift_hip_match_list_codes_batched",
         "sift_hip_match_list_host", "sift_hip_default_match_filter")


def test_entry_points_exported_with_documented_signatures(sift, tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libsift_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    for name in NAMES:
        assert name in exported, name
        assert getattr(sift.lib(), name).argtypes is not None
    src = tmp_path / "signatures.c"
    src.write_text(SIGNATURES)
    # a C compile of the header: a function pointer of another type is an error
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    L = sift.lib()
    assert len(L.sift_hip_match_list_device.argtypes) == 9
    assert len(L.sift_hip_match_list_batched.argtypes) == 10
    assert len(L.sift_hip_match_list_codes_batched.argtypes) == 14
    assert len(L.sift_hip_match_list_host.argtypes) == 9


def test_record_and_filter_layout(sift):
    assert sift.DMATCH_DTYPE.itemsize == 16
    assert sift.DMATCH_DTYPE.names == ("queryIdx", "trainIdx", "imgIdx", "distance")
    assert [sift.DMATCH_DTYPE.fields[n][1] for n in sift.DMATCH_DTYPE.names] == [0, 4, 8, 12]
    assert ctypes.sizeof(sift._MatchFilter) == 20
    f = sift._MatchFilter(9.0, 9, 9, 9.0, 9)
    sift.lib().sift_hip_default_match_filter(ctypes.byref(f))
    assert (round(f.ratio, 6), f.ratio_on_squared, f.ratio_both_ways, f.max_distance, f.cross_check) == (0.8, 0, 0, 0.0, 1)
    g = sift._match_filter()  # the Python keywords' defaults are the C defaults
    assert bytes(g) == bytes(f)


def test_surfaces_exist(sift):
    import inspect

    from sift_amd import cv

    for name in ("match_list_device", "match_list_batched", "match_list_codes_batched", "match_list_host"):
        assert callable(getattr(sift.Matcher, name)), name
    assert "filter" in inspect.signature(sift.matchList).parameters
    assert callable(cv.filter_matches) and callable(cv.to_cv_dmatches)
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIBDIR, "libsift_cuda.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "sift_cuda::matchList(sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, " \
           "sift_cuda::DeviceBuffer<sift_cuda::Half> const&, int, sift_cuda::MatchFilter const&)" in out


def test_null_arguments_are_invalid(sift):
    L = sift.lib()
    f = sift._match_filter()
    buf = np.zeros(64, np.int32)
    one = ctypes.c_int(1)
    p = ctypes.c_void_p(buf.ctypes.data)
    n = ctypes.c_int(-7)
    assert L.sift_hip_match_list_device(None, buf.ctypes.data, 1, buf.ctypes.data, 1, ctypes.byref(f), buf.ctypes.data,
                                        buf.ctypes.data, None) == -1  # SIFT_HIP_ERR_INVALID
    assert L.sift_hip_match_list_batched(None, 1, ctypes.byref(p), ctypes.byref(one), ctypes.byref(p), ctypes.byref(one),
                                         ctypes.byref(f), buf.ctypes.data, buf.ctypes.data, None) == -1
    assert L.sift_hip_match_list_codes_batched(None, buf.ctypes.data, buf.ctypes.data, 1, ctypes.byref(one),
                                               ctypes.byref(one), ctypes.byref(one), ctypes.byref(one), ctypes.byref(one),
                                               ctypes.byref(one), ctypes.byref(f), buf.ctypes.data, buf.ctypes.data,
                                               None) == -1
    assert L.sift_hip_match_list_host(None, buf.ctypes.data, 1, buf.ctypes.data, 1, ctypes.byref(f), buf.ctypes.data, 1,
                                      ctypes.byref(n)) == -1
    assert b"match" in L.sift_hip_last_error() or L.sift_hip_last_error()


# ---- cv.filter_matches against the rule stated by brute force --------------------------------------------------

def top2(q, t):
    """(nq, 2) indices and squared distances, ties to the lower train index, -1 / FLT_MAX where there is none."""
    idx = np.full((len(q), 2), -1, np.int32)
    d2 = np.full((len(q), 2), np.finfo(np.float32).max, np.float32)
    for i, row in enumerate(q):
        cand = sorted((float(((row - tr) ** 2).sum()), j) for j, tr in enumerate(t))[:2]
        for k, (d, j) in enumerate(cand):
            idx[i, k], d2[i, k] = j, d
    return idx, d2


def brute_force_list(q, t, ratio, squared, both, maxd, cross):
    """The rule of include/sift_hip.h, one query at a time, from the distance matrix itself."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    D = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1) if len(q) and len(t) else np.zeros((len(q), len(t)))

    def pass_ratio(dists):  # dists: one row's distances to the other set, in index order
        order = sorted(range(len(dists)), key=lambda j: (dists[j], j))
        if not order:
            return False
        if len(order) == 1 or not ratio > 0:
            return True
        d1, d2 = np.float32(dists[order[0]]), np.float32(dists[order[1]])
        if squared:
            return bool(d1 < np.float32(ratio) * d2)
        return bool(np.sqrt(d1) < np.float32(ratio) * np.sqrt(d2))

    out = []
    for i in range(len(q)):
        if not len(t):
            continue
        i1 = min(range(len(t)), key=lambda j: (D[i, j], j))
        if not pass_ratio(D[i]):
            continue
        dist = np.sqrt(np.float32(D[i, i1]))
        if maxd > 0 and not dist <= np.float32(maxd):
            continue
        if cross and min(range(len(q)), key=lambda k: (D[k, i1], k)) != i:
            continue
        if both and not pass_ratio(D[:, i1]):
            continue
        out.append((i, i1, 0, dist))
    return out


def desc(rows):
    """Tiny 128-D integer descriptors from their first few coordinates."""
    out = np.zeros((len(rows), 128), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


CASES = {
    # q0's nearest is t0, but t0's nearest is q1: q0 is dropped by the cross check, kept without it
    "triangle": (desc([[10, 0], [13, 0], [40, 40]]), desc([[14, 0], [41, 41], [90, 90]])),
    # duplicate rows in both sets: exact ties in both directions (lower index wins) and d1 == d2 in the ratio test
    "duplicates": (desc([[5, 5], [5, 5], [20, 1], [20, 1], [7, 9]]), desc([[5, 6], [5, 6], [20, 0], [5, 5], [20, 0], [5, 5]])),
    "one_train_row": (desc([[1, 2], [3, 4], [50, 60]]), desc([[3, 3]])),
    "one_query_row": (desc([[3, 3]]), desc([[1, 2], [3, 4], [50, 60]])),
    "empty_train": (desc([[1, 2], [3, 4]]), desc([])),
    "empty_query": (desc([]), desc([[1, 2], [3, 4]])),
    "mixed": (desc([[0, 0], [10, 0], [10, 1], [30, 30], [31, 30], [100, 0]]),
              desc([[10, 0], [0, 1], [30, 31], [99, 0], [98, 0], [200, 200]])),
}
FILTERS = [dict(ratio=r, ratio_on_squared=s, ratio_both_ways=b, max_distance=m, cross_check=c)
           for r, s, b, m, c in itertools.product((0.0, 0.8, 0.95), (False, True), (False, True), (0.0, 1.5), (False, True))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_filter_matches_is_the_rule(sift, name):
    from sift_amd import cv

    q, t = CASES[name]
    fi, fd = top2(q, t)
    ri, rd = top2(t, q)
    for f in FILTERS:
        got = cv.filter_matches(fi, fd, ri, rd, **f)
        assert got.dtype == sift.DMATCH_DTYPE
        exp = brute_force_list(q, t, f["ratio"], f["ratio_on_squared"], f["ratio_both_ways"], f["max_distance"],
                               f["cross_check"])
        assert [tuple(r) for r in got.tolist()] == [(a, b, c, float(d)) for a, b, c, d in exp], (name, f)


def test_filter_matches_named_outcomes(sift):
    from sift_amd import cv

    q, t = CASES["triangle"]
    fi, fd = top2(q, t)
    ri, rd = top2(t, q)
    assert fi[0, 0] == 0 and ri[0, 0] == 1  # the non-mutual triangle
    assert cv.filter_matches(fi, fd, ri, rd, ratio=0)["queryIdx"].tolist() == [1, 2]
    assert cv.filter_matches(fi, fd, ratio=0, cross_check=False)["queryIdx"].tolist() == [0, 1, 2]
    # ties: both copies of a duplicated query name the lower train duplicate; the reverse names the lower query
    q, t = CASES["duplicates"]
    fi, fd = top2(q, t)
    ri, rd = top2(t, q)
    assert fi[:2, 0].tolist() == [3, 3] and ri[3, 0] == 0
    got = cv.filter_matches(fi, fd, ri, rd, ratio=0)
    assert got["queryIdx"].tolist() == [0, 2] and got["trainIdx"].tolist() == [3, 2]
    # d1 == d2 (a duplicated train row) fails a ratio test below 1 and the records carry sqrt(e1), imgIdx as given
    assert cv.filter_matches(fi, fd, ri, rd, ratio=0.8)["queryIdx"].tolist() == []
    got = cv.filter_matches(fi, fd, ri, rd, ratio=0, cross_check=False, img_idx=5)
    assert got["imgIdx"].tolist() == [5] * 5
    assert np.array_equal(got["distance"], np.sqrt(np.float32([0, 0, 1, 1, 13])))
    # nt == 1: the one row passes every ratio test, and one query is its mutual neighbour
    q, t = CASES["one_train_row"]
    fi, fd = top2(q, t)
    ri, rd = top2(t, q)
    assert cv.filter_matches(fi, fd, ri, rd, cross_check=False)["trainIdx"].tolist() == [0, 0, 0]
    assert cv.filter_matches(fi, fd, ri, rd)["queryIdx"].tolist() == [1]
    with pytest.raises(ValueError):
        cv.filter_matches(fi, fd)  # the cross check needs the reverse arrays
