"""The reference of the batched guided-matching tests, checked on the CPU (tests/guided_batched_cases.py): the batch has
the shapes the kernels branch on, its degenerate pairs are empty by sift_amd.cv.geometry_usable, and every pair that
is large enough exercises both branches of the ratio rule."""
import numpy as np
import pytest

import epipolar_cases as ec
import guided_batched_cases as bc
import guided_cases as gc


def test_geometry_usable():
    from sift_amd import cv

    F = ec.fundamental()
    assert cv.geometry_usable(F) and cv.geometry_usable(F.reshape(-1)) and cv.geometry_usable(F * np.float32(1e-30))
    assert not cv.geometry_usable(np.zeros(9)) and not cv.geometry_usable(-np.zeros((3, 3), np.float32))
    one = np.zeros(9, np.float32)
    one[8] = 1e-45  # a denormal is not zero
    assert cv.geometry_usable(one)
    for bad in (np.inf, -np.inf, np.nan):
        G = F.copy()
        G[0, 2] = bad
        assert not cv.geometry_usable(G)
    for kind in bc.DEGENERATE:
        assert not cv.geometry_usable(bc.degenerate_F(kind)), kind
    with pytest.raises(ValueError):
        cv.geometry_usable(np.zeros(8))


def test_the_batch_has_the_documented_shapes():
    assert bc.SHAPES == [(1, 1), (1, 40), (40, 1), (33, 31), (257, 300), (300, 257), (600, 1100), (0, 50), (50, 0)]
    assert bc.SHAPES[:7] == list(gc.SHAPES)
    for kind, extra in (("window", 0), ("epipolar", 3)):
        pairs = bc.batch(kind)
        assert [(len(p["q"]), len(p["t"])) for p in pairs] == bc.SHAPES + [(33, 31)] * extra
        for p in pairs:
            assert len(p["q_xy"]) == len(p["q"]) and len(p["t_xy"]) == len(p["t"])
            assert p["fwd"][0].shape == (len(p["q"]), 2) and p["rev"][0].shape == (len(p["t"]), 2)
    # seeds differ per pair: two pairs of one shape would not hold the same rows
    assert len(set(bc.WINDOW_SEEDS)) == len(bc.SHAPES) and len(set(bc.EPIPOLAR_SEEDS)) == len(bc.SHAPES) + 3
    # the scale constants have no factor of two between any two of the first nine: the bytes of F differ per pair
    Fs = [p["F"].tobytes() for p in bc.epipolar_batch()]
    assert len(set(Fs)) == len(Fs)
    for a in range(len(bc.SHAPES)):
        for b in range(a):
            r = bc.SCALES[a] / bc.SCALES[b]
            assert np.log2(r) != np.rint(np.log2(r)), (a, b)


def test_degenerate_pairs_are_empty():
    pairs = bc.epipolar_batch()
    for p in pairs[:len(bc.SHAPES)]:
        assert p["usable"]
    lists = bc.expected_lists("epipolar")
    for p, got in zip(pairs[len(bc.SHAPES):], lists[len(bc.SHAPES):]):
        assert not p["usable"]
        assert np.all(p["fwd"][0] == -1) and np.all(p["fwd"][1] == bc.FLT_MAX)
        assert np.all(p["rev"][0] == -1) and np.all(p["rev"][1] == bc.FLT_MAX)
        assert len(got) == 0
    # under the formula alone a zero F would make every row a candidate: the rule is not redundant
    from sift_amd import cv

    z = pairs[len(bc.SHAPES)]
    assert cv.epipolar_mask(z["q_xy"], z["t_xy"], z["F"], ec.MAX_ERROR).all()
    idx2, d2, match = bc.expected_top2("epipolar")
    assert np.all(idx2[-99:] == -1) and np.all(d2[-99:] == bc.FLT_MAX) and np.all(match[-99:] == -1)


@pytest.mark.parametrize("kind", ["window", "epipolar"])
def test_both_branches_of_the_ratio_rule(kind):
    """Every non-empty, non-degenerate pair of at least 33 queries and two train rows has a query with two or more candidates (the ratio
    test runs) and one with none (-1); somewhere a query has exactly one (it matches without a test)."""
    from sift_amd import cv

    single = False
    seen = 0
    for p in bc.batch(kind):
        nq, nt = len(p["q"]), len(p["t"])
        if not nq or not nt or not p.get("usable", True):
            continue
        if kind == "window":
            cand = cv.gate_mask(p["q_xy"], p["t_xy"], gc.RADIUS)
        else:
            cand = cv.epipolar_mask(p["q_xy"], p["t_xy"], p["F"], ec.MAX_ERROR)
        n = cand.sum(1)
        assert np.array_equal(n >= 1, p["fwd"][0][:, 0] >= 0) and np.array_equal(n >= 2, p["fwd"][0][:, 1] >= 0)
        single |= bool((n == 1).any())
        if nq >= 33 and nt >= 2:  # (40, 1) has one train row: no query of it can have two candidates
            seen += 1
            assert (n >= 2).any() and (n == 0).any(), (kind, nq, nt)
    assert single and seen == 4
    lists = bc.expected_lists(kind)
    big = bc.SHAPES.index((600, 1100))
    assert 0 < len(lists[big]) < 600 and np.all(lists[big]["imgIdx"] == big)
    assert len(lists[bc.SHAPES.index((0, 50))]) == 0 and len(lists[bc.SHAPES.index((50, 0))]) == 0
    # the filter's other settings keep something too, and not the same
    loose = bc.expected_lists(kind, cross_check=False)
    assert len(loose[big]) > len(lists[big])
    assert 0 < len(bc.expected_lists(kind, ratio_both_ways=True, max_distance=30.0)[big]) <= len(lists[big])


def test_geometry_records():
    for stride in (36, 52):
        rec = bc.geometry_records(stride)
        assert rec.shape == (12, stride // 4) and rec.dtype == np.uint32
        for i, p in enumerate(bc.epipolar_batch()):
            assert rec[i, :9].tobytes() == p["F"].tobytes()
        assert np.all(rec[:, 9:] == 0x7FC00123)
