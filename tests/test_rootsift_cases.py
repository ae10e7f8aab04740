"""The RootSIFT rule in numpy (sift_amd.cv.rootsift, the mirror of include/sift_hip.h's rule and of
csrc/sift_rootsift.h) on hand-made rows and on the golden descriptors.  CPU only."""
import os

import numpy as np
import pytest

from sift_amd import cv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera256.npz")


def row(entries=None, fill=0):
    r = np.full(128, fill, np.float32)
    for i, v in (entries or {}).items():
        r[i] = v
    return r


def test_zero_row_stays_zero():
    out = cv.rootsift(np.zeros((2, 128), np.uint8))
    assert out.dtype == np.uint8 and out.shape == (2, 128) and not out.any()


def test_one_hot_row_clamps():
    out = cv.rootsift(row({5: 200})[None])
    assert out[0, 5] == 255 and out[0].sum() == 255  # 512 * sqrt(1) = 512: the clamp of step 5


def test_equal_bytes():
    for b in (1, 7, 255):
        out = cv.rootsift(row(fill=b)[None])
        assert (out == 45).all(), b  # cvRound(512 / sqrt(128)) = cvRound(45.25)


def test_fp16_inputs_round_and_clamp():
    """Step 1 on non-integer and non-finite fp16 inputs: round half even, clamp to 0..255, NaN -> 0."""
    v = np.zeros((1, 128), np.float16)
    v[0, :7] = [0.5, 1.5, 254.5, 255.5, -3, np.nan, np.inf]
    b = np.array([0, 2, 254, 255, 0, 0, 255], np.int32)  # 255.5 -> 256 -> 255
    want = np.zeros(128, np.uint8)
    s = np.float32(b.sum())
    want[:7] = np.minimum(np.rint(np.float32(512) * np.sqrt(b.astype(np.float32) / s)), 255)
    got = cv.rootsift(v)
    assert np.array_equal(got[0], want)
    # the same bytes handed in as integers give the same row: step 1 is all that differs
    ints = np.zeros((1, 128), np.uint8)
    ints[0, :7] = b
    assert np.array_equal(cv.rootsift(ints), got)


def test_shape_is_checked():
    with pytest.raises(ValueError):
        cv.rootsift(np.zeros(128, np.uint8))
    with pytest.raises(ValueError):
        cv.rootsift(np.zeros((2, 64), np.uint8))


def test_golden_rows():
    d = np.load(GOLD)["default_desc"]
    r = cv.rootsift(d)
    assert len(d) > 100 and r.max() < 255, "no byte clamps"
    nrm = np.linalg.norm(r.astype(np.float64), axis=1)
    print(f"norms {nrm.min():.1f} .. {nrm.max():.1f}, largest byte {r.max()}")
    assert nrm.min() >= 505 and nrm.max() <= 520
    # the rule is monotone per row: the largest entry stays the largest
    am = d.argmax(axis=1)
    assert np.array_equal(r[np.arange(len(r)), am], r.max(axis=1))
    assert np.array_equal(cv.rootsift(d.astype(np.float16)), r) and np.array_equal(cv.rootsift(d.astype(np.float32)), r)
