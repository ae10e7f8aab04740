"""The inputs of tests/test_gpu_match_general.py (tests/general_cases.py) against their float64 / int64 references
alone, on the CPU: the conditions under which the GPU tests mean something."""
import numpy as np
import pytest

import general_cases as gc

DIRECTIONS = ("fwd", "rev")


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_values_take_the_general_path_and_round(family):
    c = gc.case(family)
    for a in (c.q, c.t):
        assert a.dtype == np.float16 and np.isfinite(a).all()
        assert np.any(a != np.rint(a))  # not an integer set
        # fp32 cannot hold the row's sum of squares exactly: partial sums need more than 24 bits
        sq = a.astype(np.float64) ** 2
        assert np.any(sq.cumsum(1).astype(np.float32) != sq.cumsum(1))
    if family == "sift_unrounded":
        n2 = (c.q.astype(np.float64) ** 2).sum(1)
        assert c.q.min() >= 0 and np.all(np.abs(n2 - 512.0 ** 2) < 0.01 * 512.0 ** 2)
    else:
        neg = (c.q < 0).mean()
        dots = c.q.astype(np.float64) @ c.t.astype(np.float64).T
        absdots = np.abs(c.q.astype(np.float64)) @ np.abs(c.t.astype(np.float64)).T
        assert 0.45 < neg < 0.55 and np.median(absdots / np.maximum(np.abs(dots), 1e-30)) > 5


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_decidable_share_and_bound(family):
    c = gc.case(family)
    for dn in DIRECTIONS:
        d = getattr(c, dn)
        for g in gc.GATES:
            share = d.ref[g].decidable.mean()
            print(f"{family} {dn} {g}: decidable {share:.4f}, candidates per query {d.cand[g].sum(1).mean():.1f}")
            assert share >= 0.95, (family, dn, g, share)
        nearest = d.ref["none"].top[:, 0]
        assert d.B.max() < 1e-3 * np.median(nearest), (family, dn, d.B.max(), np.median(nearest))


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_planted_rows(family):
    c = gc.case(family)
    (q1, t1), (q0, (ta, tb)), (q2, tl) = gc.DUP_SINGLE, gc.DUP_DOUBLE, gc.DUP_LAST
    assert tl == gc.NT - 1 and gc.NT % 32 != 0  # the last, partial tile
    assert ta // 256 != tb // 256 and ta // 128 != tb // 128  # different splits of every kernel
    for g in gc.GATES:  # the duplicates are the float64 nearest neighbours, at D = 0, under every gate
        e, top = c.fwd.ref[g].expect, c.fwd.ref[g].top
        assert e[q0].tolist() == [ta, tb] and top[q0, 0] == 0 and top[q0, 1] == 0 and top[q0, 2] > 0
        assert e[q1, 0] == t1 and top[q1, 0] == 0 and top[q1, 1] > 0
        assert e[q2, 0] == tl and top[q2, 0] == 0 and top[q2, 1] > 0
        r = c.rev.ref[g].expect
        assert r[t1, 0] == q1 and r[ta, 0] == q0 and r[tb, 0] == q0 and r[tl, 0] == q2
    assert c.t[ta].tobytes() == c.t[tb].tobytes() == c.q[q0].tobytes()
    # the noisy copies: nearest neighbours, not duplicates, inside both gates
    src, dst = c.planted[:, 0], c.planted[:, 1]
    assert len(src) == 150 and len(set(src)) == 150 and len(set(dst)) == 150
    assert np.array_equal(c.fwd.ref["none"].expect[src, 0], dst) and np.all(c.fwd.D[src, dst] > 0)
    assert c.fwd.cand["window"][src, dst].all() and c.fwd.cand["band"][src, dst].all()


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_gates_are_real(family):
    c = gc.case(family)
    for dn in DIRECTIONS:
        d = getattr(c, dn)
        n = d.D.shape[1]
        assert 0.05 * n < d.cand["window"].sum(1).mean() < 0.5 * n
        assert 1 < d.cand["band"].sum(1).mean() < 0.1 * n
        for g in ("window", "band"):  # the gate changes the answer of most queries
            assert (d.ref[g].expect[:, 0] != d.ref["none"].expect[:, 0]).mean() > 0.3
    assert np.array_equal(c.rev.cand["window"], c.fwd.cand["window"].T)


def test_analyse_and_measure_on_a_hand_case():
    """Three train rows at distances 0, 1 and 1 + tiny of the one query: the first is pinned, the order of the other
    two is not; measure_top2 accepts either order and flags a negative distance, a NaN and a wrong first index."""
    D = np.array([[1.0 + 1e-9, 0.0, 1.0]])
    B = np.full((1, 3), 1e-6)
    cand = np.ones((1, 3), bool)
    ref = gc.analyse(D, B, cand)
    assert ref.expect.tolist() == [[1, 2]] and not ref.decidable[0]
    for idx in ([[1, 2]], [[1, 0]]):
        stats, bad = gc.measure_top2(np.int32(idx), np.float32([[0.0, 1.0]]), D, B, cand)
        assert all(len(v) == 0 for v in bad.values()), bad
    _, bad = gc.measure_top2(np.int32([[1, 2]]), np.float32([[-1e-7, 1.0]]), D, B, cand)
    assert len(bad["negative"]) == 1
    _, bad = gc.measure_top2(np.int32([[1, 2]]), np.float32([[np.nan, 1.0]]), D, B, cand)
    assert len(bad["nan"]) == 1 and len(bad["bound"]) == 1
    _, bad = gc.measure_top2(np.int32([[0, 2]]), np.float32([[1.0, 1.0]]), D, B, cand)
    assert len(bad["index"]) == 1
    _, bad = gc.measure_top2(np.int32([[1, 1]]), np.float32([[0.0, 0.0]]), D, B, cand)
    assert len(bad["distinct"]) == 1
    wide = gc.analyse(np.array([[5.0, 0.0, 1.0]]), B, cand)
    assert wide.decidable[0]
    _, bad = gc.measure_top2(np.int32([[1, 0]]), np.float32([[0.0, 5.0]]), np.array([[5.0, 0.0, 1.0]]), B, cand, wide)
    assert len(bad["decidable"]) == 1
    none = np.zeros((1, 3), bool)
    _, bad = gc.measure_top2(np.int32([[-1, -1]]), np.float32([[gc.FLT_MAX, gc.FLT_MAX]]), D, B, none)
    assert all(len(v) == 0 for v in bad.values())
    _, bad = gc.measure_top2(np.int32([[1, -1]]), np.float32([[0.0, gc.FLT_MAX]]), D, B, none)
    assert len(bad["none"]) == 1


def test_fullrange_sets():
    f = gc.fullrange()
    ext = gc.extreme_rows()
    for a in (f.q, f.t):
        assert a.min() == 0 and a.max() == 255 and np.all(a == np.rint(a))
    sparse = f.t[np.setdiff1d(np.arange(gc.NT // 2, gc.NT), list(gc.TRAIN_EXTREMES))]  # the second half of the rows
    assert 0.55 < (sparse == 0).mean() < 0.65 and sparse.max() == 150
    for i, name in gc.TRAIN_EXTREMES.items():
        assert np.array_equal(f.t[i], ext[name])
    for i, name in gc.QUERY_EXTREMES.items():
        assert np.array_equal(f.q[i], ext[name])
    assert {255, 511, gc.NT - 1} <= set(gc.TRAIN_EXTREMES) and 255 % 256 == 255 and 511 % 256 == 255
    for name in ext:  # every kind twice, in different key-group splits of the pair kernels
        at = [i for i, n in gc.TRAIN_EXTREMES.items() if n == name]
        assert len({i // 256 for i in at}) >= 2, name
    # the ungated int64 reference holds the extreme duplicates ...
    idx, d2 = f.fwd["none"]
    assert idx[0].tolist() == [511, 767] and d2[0].tolist() == [0, 0]
    assert idx[1].tolist() == [255, gc.NT - 1] and d2[1].tolist() == [0, 0]
    assert idx[2].tolist() == [256, 1023] and idx[3].tolist() == [300, 900] and idx[4].tolist() == [100, 1050]
    assert np.all(d2[:5] == 0) and idx[256].tolist() == [511, 767] and idx[gc.NQ - 1].tolist() == [255, gc.NT - 1]
    # ... and the gated ones the largest distance two codes can have, as a tie across splits
    for g in ("window", "band"):
        idx, d2 = f.fwd[g]
        assert idx[gc.FAR].tolist() == [255, gc.NT - 1] and d2[gc.FAR].tolist() == [gc.MAX_D2, gc.MAX_D2]
        assert d2[idx >= 0].max() == gc.MAX_D2
        ridx, rd2 = f.rev[g]
        for row in (255, gc.NT - 1):
            assert ridx[row].tolist() == [gc.FAR, -1] and rd2[row, 0] == gc.MAX_D2
    assert gc.MAX_D2 == 8323200
    # a zero to turn into -0.0 in the general-path variant
    assert f.q[gc.MINUS_ZERO_QUERY, 17] == 0 and f.t[gc.MINUS_ZERO_TRAIN, 90] == 0
