"""The gated k-NN mirrors (sift_amd.cv.mask_knn, guided_knn, epipolar_knn) and the shared case set, on the CPU.

The mirrors against a double loop over the candidates; their identities (no gate = cv.knn, k = 2 = the gated top-2,
the column prefix); and the conditions the GPU tests rely on: the case set holds queries with 0, 1, k - 1, k, k + 1
and >= 2k candidates for every served k under both gates, and the planted ties sit where the docstring says.
"""
import numpy as np
import pytest

import knn_cases as kc
import knn_gated_cases as kg


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def prefix(table, k):
    return np.ascontiguousarray(table[0][:, :k]), np.ascontiguousarray(table[1][:, :k])


@pytest.mark.parametrize("gate", kg.GATES)
@pytest.mark.parametrize("nq,nt,k", [s for s in kc.SHAPES if s[:2] != kc.BIG])
def test_mirror_is_the_brute_force(sift, gate, nq, nt, k):
    q, t = kc.sets(nq, nt)
    q_xy, t_xy = kg.positions(nq, nt)
    cand = kg.mask(gate, q_xy, t_xy)
    assert same(kg.reference(gate, nq, nt, k), kg.brute_force(q, t, cand, k))


@pytest.mark.parametrize("gate", kg.GATES)
def test_mirror_on_the_big_shape_rows_that_matter(sift, gate):
    q, t = kc.sets(*kc.BIG)
    q_xy, t_xy = kg.positions(*kc.BIG)
    rows = [0, 1, 2, kg.FAR_QUERY, kg.NAN_QUERY, kg.CLUSTER_QUERY, 299]
    cand = kg.mask(gate, q_xy, t_xy)
    ref = kg.reference(gate, *kc.BIG, 8)
    bf = kg.brute_force(q[rows], t, cand[rows], 8)
    assert same((ref[0][rows], ref[1][rows]), bf)
    assert (ref[0][[kg.FAR_QUERY, kg.NAN_QUERY]] == -1).all() and (ref[1][[kg.FAR_QUERY, kg.NAN_QUERY]] == kg.FLT_MAX).all()
    assert set(ref[0][kg.CLUSTER_QUERY].tolist()) <= set(np.flatnonzero(cand[kg.CLUSTER_QUERY]).tolist())
    assert (ref[0][kg.CLUSTER_QUERY] >= 0).all()
    assert not (ref[0] == kg.NAN_TRAIN).any() and not cand[:, kg.NAN_TRAIN].any()


def test_no_gate_is_knn(sift):
    from sift_amd import cv

    for nq, nt, k in kc.SHAPES:
        q, t = kc.sets(nq, nt)
        q_xy, t_xy = kg.positions(nq, nt)
        if (nq, nt) == kc.BIG:  # a NaN coordinate is a candidate of nothing even without a window
            q_xy, t_xy = np.nan_to_num(q_xy, nan=1.0), np.nan_to_num(t_xy, nan=1.0)
        assert same(cv.guided_knn(q, t, q_xy, t_xy, np.inf, k), kc.reference(nq, nt, k)), (nq, nt, k)
        assert same(cv.epipolar_knn(q, t, q_xy, t_xy, kg.F, 1e30, k), kc.reference(nq, nt, k)), (nq, nt, k)
    q, t = kc.low_entropy()
    assert same(cv.mask_knn(q, t, np.ones((len(q), len(t)), bool), 8), cv.knn(q, t, 8))


def test_k2_is_the_gated_top2(sift):
    from sift_amd import cv

    for (q, t), (q_xy, t_xy) in ((kc.sets(*kc.BIG), kg.positions(*kc.BIG)), (kc.tie_sets(), kg.tie_positions("a")),
                                 (kg.half_sets(), kg.positions(70, 300))):
        assert same(cv.guided_knn(q, t, q_xy, t_xy, kg.RADIUS, 2), cv.guided_top2(q, t, q_xy, t_xy, kg.RADIUS))
        assert same(cv.epipolar_knn(q, t, q_xy, t_xy, kg.F, kg.MAX_ERROR, 2),
                    cv.epipolar_top2(q, t, q_xy, t_xy, kg.F, kg.MAX_ERROR))
        cand = kg.mask("band", q_xy, t_xy) & kg.mask("window", q_xy, t_xy)
        assert same(cv.mask_knn(q, t, cand, 2), cv.mask_top2(q, t, cand))
        assert same(cv.epipolar_knn(q, t, q_xy, t_xy, kg.F, kg.MAX_ERROR, 2, radius=kg.RADIUS), cv.mask_top2(q, t, cand))


@pytest.mark.parametrize("gate", kg.GATES)
def test_column_prefix(sift, gate):
    wide = kg.reference(gate, *kc.BIG, 8)
    for k in kg.KS:
        assert same(kg.reference(gate, *kc.BIG, k), prefix(wide, k)), k


@pytest.mark.parametrize("gate", kg.GATES)
def test_candidate_counts_straddle_every_k(sift, gate):
    """A condition on the inputs, not a measurement."""
    counts = kg.mask(gate, *kg.positions(*kc.BIG)).sum(1)
    have = set(counts.tolist())
    for k in kg.KS:
        for c in (0, 1, k - 1, k, k + 1):
            assert c in have, (gate, k, c)
        assert (counts >= 2 * k).any(), (gate, k)
    assert counts[kg.FAR_QUERY] == 0 and counts[kg.NAN_QUERY] == 0
    assert counts[kg.CLUSTER_QUERY] >= 2 * kc.KNN_MAX
    # the small shapes' windows are not all empty either
    for nq, nt, _ in kc.SHAPES:
        assert kg.mask(gate, *kg.positions(nq, nt)).any() or (nq, nt) == (1, 1) or gate == "band", (gate, nq, nt)


@pytest.mark.parametrize("gate", kg.GATES)
@pytest.mark.parametrize("variant", ("a", "b"))
def test_planted_ties(sift, gate, variant):
    from sift_amd import cv

    q, t = kc.tie_sets()
    q_xy, t_xy = kg.tie_positions(variant)
    cand = kg.mask(gate, q_xy, t_xy)
    inside = sorted(kg.TIE_INSIDE[variant])
    assert [r for r in kc.TIE_ROWS if cand[0, r]] == [r for r in kc.TIE_ROWS if r in inside]
    assert cand[0, 255] == (variant == "a") and cand[0, 256] == (variant == "b")
    idx, d2 = kg.mirror(gate, q, t, q_xy, t_xy, 8)
    assert idx[0, :len(inside)].tolist() == inside and not d2[0, :len(inside)].any()
    assert len(inside) == 7 and d2[0, 7] > 0  # the eighth entry is a real neighbour, not a copy outside the gate
    assert set(kc.TIE_ROWS) - set(inside) and not np.isin(idx[0], sorted(set(kc.TIE_ROWS) - set(inside))).any()
    # cut where the plan splits: rows 255 and 256 straddle the key group and the split
    assert same(kg.mirror(gate, q, t[:257], q_xy, t_xy[:257], 8), kg.brute_force(q, t[:257], cand[:, :257], 8))
    assert same(cv.mask_knn(q, t, lambda: cand, 3), cv.mask_knn(q, t, cand, 3))


def test_exact_half_values(sift):
    """Multiples of 0.5 go through the float64 form and stay exact: the general path is compared byte for byte."""
    from sift_amd import cv

    q, t = kg.half_sets()
    q_xy, t_xy = kg.positions(70, 300)
    for gate in kg.GATES:
        cand = kg.mask(gate, q_xy, t_xy)
        idx, d2 = kg.mirror(gate, q, t, q_xy, t_xy, 8)
        exact = ((q[:, None, :].astype(np.float64) - t[None, :, :]) ** 2).sum(-1)
        rows = np.arange(len(q))[:, None]
        ok = idx >= 0
        assert (np.where(ok, exact[rows, np.maximum(idx, 0)], kg.FLT_MAX).astype(np.float32) == d2).all()
        assert (ok.sum(1) == np.minimum(cand.sum(1), 8)).all()
    # special values: a query row with NaN has no neighbour, a train row with inf is nobody's
    qs, ts = q.copy(), t.copy()
    qs[7, 3] = np.nan
    ts[40, 9] = np.inf
    idx, d2 = cv.mask_knn(qs, ts, np.ones((70, 300), bool), 8)
    assert (idx[7] == -1).all() and (d2[7] == kg.FLT_MAX).all() and not (idx == 40).any()
    with pytest.raises(ValueError):
        cv.mask_knn(q, t, np.ones((70, 300), bool), 9)
