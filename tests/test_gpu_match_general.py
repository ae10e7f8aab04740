"""The matcher's general (fp16) path where fp32 rounds, and full-range codes on both paths.

The contract is the "general path" paragraph of include/sift_hip.h, items 1 to 7; the inputs and the float64 / int64
references are tests/general_cases.py (checked on the CPU by tests/test_match_general_cases.py).  Every route of a
single pair is run once per family and shared by the tests below:

    device      match_device                       k_match_single, 9 splits of 4 tiles
    batched1    match_batched, one pair            the same kernel
    batched     match_batched, both directions     k_match_prep + k_match_batch, key-group splits
    guided_open match_guided_device, radius inf    k_match_guided, every row a candidate
    epi_open    match_epipolar_device, 1e30        k_match_epipolar, every row a candidate
    window      match_guided_device at RADIUS
    band        match_epipolar_device at MAX_ERROR

"fwd" is q against t, "rev" t against q (positions swapped, F transposed).
"""
import numpy as np
import pytest

import general_cases as gc

pytestmark = pytest.mark.gpu
INF = float("inf")
OPEN = ("device", "batched1", "batched", "batched_second", "guided_open", "epi_open")  # all rows candidates
GATE_OF = {**{r: "none" for r in OPEN}, "window": "window", "band": "band"}
CAP = max(gc.NQ, gc.NT)


def upload(sift, rows):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(np.asarray(rows).astype(np.float16)).view(np.uint16))


def same(got, ref):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, ref))


def ratio_match(idx2, d2):
    """The `match` output (ratio 0.8 on distances) from a top-2."""
    from sift_amd import cv

    return np.where(cv._ratio_pass(idx2, d2, 0.8, False), idx2[:, 0], -1).astype(np.int32)


class Side:
    """One descriptor set on the device with its positions."""

    def __init__(self, sift, rows, xy):
        self.n = len(rows)
        self.rows, self.xy = upload(sift, rows), sift.DeviceArray.from_numpy(np.ascontiguousarray(xy, np.float32))


class Pair:
    """A query and a train side, F, and the calls of every route; outputs start as a pattern the kernel overwrites."""

    def __init__(self, sift, m, a, b, F, band_radius=INF):
        self.sift, self.m, self.a, self.b, self.F, self.band_radius = sift, m, a, b, np.ascontiguousarray(F), band_radius

    def swapped(self):
        return Pair(self.sift, self.m, self.b, self.a, self.F.T, self.band_radius)

    def _top2(self, n, call):
        s = self.sift
        idx2 = s.DeviceArray.from_numpy(np.full(2 * n, -77, np.int32))
        d2 = s.DeviceArray.from_numpy(np.full(2 * n, -77, np.float32))
        mt = s.DeviceArray.from_numpy(np.full(n, -77, np.int32))
        call(idx2.value, d2.value, mt.value)
        return idx2.to_numpy(np.int32, (n, 2)), d2.to_numpy(np.float32, (n, 2)), mt.to_numpy(np.int32, (n,))

    def run(self, route):
        a, b, m = self.a, self.b, self.m
        av, bv, axy, bxy = a.rows.value, b.rows.value, a.xy.value, b.xy.value
        if route == "device":
            return self._top2(a.n, lambda i, d, t: m.match_device(av, a.n, bv, b.n, 0.8, False, i, d, t))
        if route == "batched1":
            return self._top2(a.n, lambda i, d, t: m.match_batched([av], [a.n], [bv], [b.n], 0.8, False, i, d, t))
        if route in ("batched", "batched_second"):  # this pair as the first / the second of two
            first = route == "batched"
            qs, ts = ([av, bv], [bv, av]) if first else ([bv, av], [av, bv])
            ns, ms = ([a.n, b.n], [b.n, a.n]) if first else ([b.n, a.n], [a.n, b.n])
            out = self._top2(a.n + b.n, lambda i, d, t: m.match_batched(qs, ns, ts, ms, 0.8, False, i, d, t))
            return tuple(o[:a.n] if first else o[b.n:] for o in out)
        if route in ("guided_open", "window"):
            r = INF if route == "guided_open" else gc.RADIUS
            return self._top2(a.n, lambda i, d, t: m.match_guided_device(av, a.n, bv, b.n, axy, bxy, r, 2, 2, 0.8, False,
                                                                         i, d, t))
        if route in ("epi_open", "band"):
            e, r = (1e30, INF) if route == "epi_open" else (gc.MAX_ERROR, self.band_radius)
            return self._top2(a.n, lambda i, d, t: m.match_epipolar_device(av, a.n, bv, b.n, axy, bxy, self.F, e, r, 2, 2,
                                                                           0.8, False, i, d, t))
        raise ValueError(route)

    def _list(self, rows, ncounts, call):
        s = self.sift
        out = s.DeviceArray.from_numpy(np.full(4 * rows, -1, np.int32))
        cnt = s.DeviceArray.from_numpy(np.full(ncounts, -1, np.int32))
        call(out.value, cnt.value)
        return out.to_numpy(s.DMATCH_DTYPE, (rows,)), cnt.to_numpy(np.int32, (ncounts,))

    def list(self, kind, **f):
        a, b, m = self.a, self.b, self.m
        av, bv, axy, bxy = a.rows.value, b.rows.value, a.xy.value, b.xy.value
        if kind == "batched":  # both directions as two pairs: [pair 0 records, pair 1 records]
            out, cnt = self._list(a.n + b.n, 2, lambda o, c: m.match_list_batched([av, bv], [a.n, b.n], [bv, av],
                                                                                  [b.n, a.n], o, c, **f))
            assert 0 <= cnt[0] <= a.n and 0 <= cnt[1] <= b.n
            return [out[:cnt[0]], out[a.n:a.n + cnt[1]]]
        if kind == "none":
            out, cnt = self._list(a.n, 1, lambda o, c: m.match_list_device(av, a.n, bv, b.n, o, c, **f))
        elif kind == "window":
            out, cnt = self._list(a.n, 1, lambda o, c: m.match_list_guided_device(av, a.n, bv, b.n, axy, bxy, gc.RADIUS,
                                                                                  o, c, 2, 2, **f))
        else:
            out, cnt = self._list(a.n, 1, lambda o, c: m.match_list_epipolar_device(
                av, a.n, bv, b.n, axy, bxy, self.F, gc.MAX_ERROR, o, c, self.band_radius, 2, 2, **f))
        assert 0 <= cnt[0] <= a.n
        return out[:cnt[0]]


_runs = {}


def runs(sift, family):
    """Every route of both directions of a family, run once: {"fwd" / "rev": {route: (idx2, d2, match)}}, and the
    Pair objects for further calls."""
    if family not in _runs:
        c = gc.case(family)
        m = sift.Matcher(CAP, CAP, 4)
        fwd = Pair(sift, m, Side(sift, c.q, c.q_xy), Side(sift, c.t, c.t_xy), c.F)
        pairs = {"fwd": fwd, "rev": fwd.swapped()}
        _runs[family] = pairs, {dn: {r: p.run(r) for r in GATE_OF} for dn, p in pairs.items()}
    return _runs[family]


def test_the_shape_splits_in_every_kernel(sift):
    assert sift.Matcher.plan(gc.NQ, gc.NT, 1)[0] == 9 and sift.Matcher.plan(gc.NT, gc.NQ, 1)[0] > 1  # k_match_single
    assert sift.Matcher.plan(CAP, CAP, 2)[0] > 1  # k_match_batch, both directions as two pairs
    assert sift.Matcher.plan(CAP, CAP, 4)[0] > 1  # the list of two pairs: four
    assert sift.Matcher.guided_plan(gc.NQ, gc.NT) > 1 and sift.Matcher.guided_plan(gc.NT, gc.NQ) > 1


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_sign_accuracy_and_indices(sift, family):
    """Items 1 to 3: no negative and no NaN d^2, |d^2 - D| <= B, the index rule for every query and the float64
    order on the decidable ones -- every route, both directions."""
    c = gc.case(family)
    _, out = runs(sift, family)
    for dn in ("fwd", "rev"):
        d = getattr(c, dn)
        for route, (idx2, d2, _) in out[dn].items():
            g = GATE_OF[route]
            gc.check_top2(idx2, d2, d.D, d.B, d.cand[g], d.ref[g], f"{family} {dn} {route}")
            assert np.isfinite(np.sqrt(d2[idx2 >= 0])).all()


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_duplicates(sift, family):
    """Item 4 and the planted rows: d^2 = 0 can come out of three differently rounded sums as a small negative
    number; the identical train rows 7 and 900 lie in different splits of every kernel and tie to the lower index."""
    _, out = runs(sift, family)
    (q1, t1), (q0, (ta, tb)), (q2, tl) = gc.DUP_SINGLE, gc.DUP_DOUBLE, gc.DUP_LAST
    for route, (idx2, d2, match) in out["fwd"].items():
        print(family, route, "query 0:", idx2[q0].tolist(), d2[q0].tolist(), "query 1:", idx2[q1].tolist(),
              d2[q1].tolist(), match[q1], "query 2:", idx2[q2].tolist(), d2[q2].tolist(), match[q2])
        assert idx2[q0].tolist() == [ta, tb], (route, idx2[q0], d2[q0])
        assert d2[q0, 0].tobytes() == d2[q0, 1].tobytes() and d2[q0, 0] >= 0, (route, d2[q0])
        assert match[q0] == -1  # the ratio test on a tie
        assert idx2[q1, 0] == t1 and match[q1] == t1, (route, idx2[q1], d2[q1], match[q1])
        assert idx2[q2, 0] == tl and match[q2] == tl, (route, idx2[q2], d2[q2], match[q2])
    for route, (idx2, d2, match) in out["rev"].items():
        for row, want in ((t1, q1), (ta, q0), (tb, q0), (tl, q2)):
            assert idx2[row, 0] == want and match[row] == want and d2[row, 0] >= 0, (route, row, idx2[row], d2[row])


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_all_routes_give_the_same_bytes(sift, family):
    """Item 5, and the open gates against the ungated kernels."""
    _, out = runs(sift, family)
    for dn in ("fwd", "rev"):
        ref = out[dn]["device"]
        for route in OPEN[1:]:
            got = out[dn][route]
            diff = np.flatnonzero((got[0] != ref[0]).any(1) | (got[1].view(np.int32) != ref[1].view(np.int32)).any(1))
            assert same(got, ref), (family, dn, route, diff[:8], got[0][diff[:4]], ref[0][diff[:4]], got[1][diff[:4]],
                                    ref[1][diff[:4]])
        for route in ("window", "band"):  # the gates do something
            assert not same(out[dn][route][:1], ref[:1])


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_match_and_lists_follow_the_returned_numbers(sift, family):
    """Item 6: `match` is the ratio rule on the returned idx2 / d2, and every list is filter_matches on the returned
    top-2 of both directions, byte for byte; the duplicates' records are there with a finite distance >= 0."""
    from sift_amd import cv

    c = gc.case(family)
    pairs, out = runs(sift, family)
    for dn in ("fwd", "rev"):
        for route, (idx2, d2, match) in out[dn].items():
            assert np.array_equal(match, ratio_match(idx2, d2)), (family, dn, route)
    cap = float(np.sqrt(np.median(c.fwd.D[c.planted[:, 0], c.planted[:, 1]])))  # about half of the noisy copies
    (q1, t1), (q2, tl) = gc.DUP_SINGLE, gc.DUP_LAST
    for gate, route in (("none", "device"), ("window", "window"), ("band", "band")):
        fwd, rev = out["fwd"][route][:2], out["rev"][route][:2]
        for f in (dict(), dict(cross_check=False), dict(max_distance=cap)):
            want = cv.filter_matches(*fwd, *rev, **f)
            got = pairs["fwd"].list(gate, **f)
            print(f"{family} {gate} {f}: kept {len(got)} (expected {len(want)})")
            assert 0 < len(want) < gc.NQ
            assert same([got], [want]), (family, gate, f, len(got), len(want))
            assert np.isfinite(got["distance"]).all() and (got["distance"] >= 0).all()
            for qi, ti in ((q1, t1), (q2, tl)):
                rec = got[got["queryIdx"] == qi]
                assert len(rec) == 1 and rec["trainIdx"][0] == ti and rec["distance"][0] >= 0, (family, gate, f, qi, rec)
        assert same([pairs["rev"].list(gate)], [cv.filter_matches(*rev, *fwd)]), (family, gate)
    fwd, rev = out["fwd"]["device"][:2], out["rev"]["device"][:2]
    got = pairs["fwd"].list("batched")
    assert same(got, [cv.filter_matches(*fwd, *rev, img_idx=0), cv.filter_matches(*rev, *fwd, img_idx=1)])


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_three_calls_give_the_same_bytes(sift, family):
    """The merge scratch is restored after an fp16 split merge: the calls after the first find it idle."""
    pairs, out = runs(sift, family)
    for dn in ("fwd", "rev"):
        for route in ("device", "batched", "window", "band"):
            for _ in range(3):
                assert same(pairs[dn].run(route), out[dn][route]), (family, dn, route)


# ---------------------------------------------------------------------------------------------------------------
# Full-range codes.
# ---------------------------------------------------------------------------------------------------------------
def fullrange_check(sift, q, t, label):
    """idx2, d2 and match of every route, both directions, and the lists against the int64 references."""
    from sift_amd import cv

    f = gc.fullrange()
    m = sift.Matcher(CAP, CAP, 4)
    fwd = Pair(sift, m, Side(sift, q, f.q_xy), Side(sift, t, f.t_xy), f.F, band_radius=gc.RADIUS)
    for dn, p in (("fwd", fwd), ("rev", fwd.swapped())):
        refs = getattr(f, dn)
        for route, gate in GATE_OF.items():
            idx2, d2, match = p.run(route)
            ref = refs[gate]
            diff = np.flatnonzero((idx2 != ref[0]).any(1) | (d2 != ref[1]).any(1))
            assert same((idx2, d2), ref), (label, dn, route, diff[:8], idx2[diff[:4]], ref[0][diff[:4]], d2[diff[:4]],
                                           ref[1][diff[:4]])
            assert np.array_equal(match, ratio_match(*ref)), (label, dn, route)
    for gate in gc.GATES:
        assert same([fwd.list(gate)], [cv.filter_matches(*f.fwd[gate], *f.rev[gate])]), (label, gate)
    assert same(fwd.list("batched"), [cv.filter_matches(*f.fwd["none"], *f.rev["none"], img_idx=0),
                                      cv.filter_matches(*f.rev["none"], *f.fwd["none"], img_idx=1)]), label


def test_fullrange_integer_path(sift):
    """Integers 0..255 with the extreme rows where the int32 keys are at the ends of their range (r = 255, the
    partial tile beside padding keys, ties across splits, d^2 = 128 * 255^2 under the gates)."""
    f = gc.fullrange()
    assert f.fwd["window"][1][gc.FAR].tolist() == [gc.MAX_D2, gc.MAX_D2]
    fullrange_check(sift, f.q, f.t, "integer")


@pytest.mark.parametrize("side", ["query", "train", "both"])
def test_fullrange_general_path(sift, side):
    """One 0 replaced by -0.0: the set is flagged (codes16) and takes the fp16 path -- in k_match_single only the
    workgroups that read the row, the others keep the integer fold -- but holds the same values.  Every sum is an
    integer below 2^24, so the bytes are the integer path's."""
    f = gc.fullrange()
    q, t = f.q.copy(), f.t.copy()
    if side in ("query", "both"):
        q[gc.MINUS_ZERO_QUERY, 17] = -0.0
    if side in ("train", "both"):
        t[gc.MINUS_ZERO_TRAIN, 90] = -0.0
    assert np.array_equal(q, f.q) and np.array_equal(t, f.t)  # the same values
    assert np.signbit(q).any() == (side != "train") and np.signbit(t).any() == (side != "query")
    assert sift.Matcher.plan(gc.NQ, gc.NT, 1)[0] == 9 and gc.MINUS_ZERO_TRAIN // 128 == 4  # one split of nine
    fullrange_check(sift, q, t, side)


@pytest.mark.parametrize("minus_zero", [False, True])
def test_largest_distance_ungated(sift, minus_zero):
    """Two all-255 train rows: the ungated top-2 of an all-0 query is d^2 = 128 * 255^2 twice, on both paths."""
    from sift_amd import cv

    ext = gc.extreme_rows()
    q = np.float32([ext["zero"], ext["full"], ext["cb"], ext["spike"]])
    t = np.float32([ext["full"], ext["full"]])
    ref = cv.mask_top2(q, t, np.ones((4, 2), bool))
    rref = cv.mask_top2(t, q, np.ones((2, 4), bool))
    assert ref[0][0].tolist() == [0, 1] and ref[1][0].tolist() == [gc.MAX_D2, gc.MAX_D2]
    if minus_zero:
        q[0, 5] = -0.0
    xy = np.float32([[10, 10], [20, 30], [50, 60], [70, 20]])
    p = Pair(sift, sift.Matcher(4, 4, 2), Side(sift, q, xy), Side(sift, t, xy[:2]), gc.ec.fundamental())
    for route in OPEN:
        assert same(p.run(route)[:2], ref), route
        assert same(p.swapped().run(route)[:2], rref), route


# ---------------------------------------------------------------------------------------------------------------
# Special values.
# ---------------------------------------------------------------------------------------------------------------
def test_special_values(sift):
    """Item 7.  NaN, +Inf and -Inf as data in train rows (one a query's duplicate, one in the partial tile) and in
    query rows: such a train row is nobody's neighbour, such a query gets (-1, -1, FLT_MAX, FLT_MAX) and match -1, and
    every other query gets the bytes of the run on the set without those train rows, indices mapped back."""
    c = gc.case("sift_unrounded")
    q, t = c.q.copy(), c.t.copy()
    tbad = {gc.DUP_SINGLE[1]: np.nan, gc.NT - 3: np.inf, 500: -np.inf, 64: np.inf}
    qbad = {10: np.nan, 20: np.inf, 30: -np.inf}
    for k, (row, v) in enumerate(tbad.items()):
        t[row, 7 + 31 * k] = v
    col = int(np.flatnonzero((c.t > 0).mean(0) > 0.5)[3])  # a column where most train rows are positive
    for row, v in qbad.items():
        q[row, col] = v
    keep = np.setdiff1d(np.arange(gc.NT), list(tbad))
    good = np.setdiff1d(np.arange(gc.NQ), list(qbad))
    m = sift.Matcher(CAP, CAP, 4)
    full = Pair(sift, m, Side(sift, q, c.q_xy), Side(sift, t, c.t_xy), c.F)
    less = Pair(sift, m, Side(sift, c.q, c.q_xy), Side(sift, c.t[keep], c.t_xy[keep]), c.F)
    for route in GATE_OF:
        idx2, d2, match = full.run(route)
        ri, rd, rm = less.run(route)
        ri, rm = np.where(ri >= 0, keep[ri], -1).astype(np.int32), np.where(rm >= 0, keep[rm], -1).astype(np.int32)
        print(route, "special queries:", idx2[list(qbad)].tolist(), d2[list(qbad)].tolist())
        assert not np.isin(idx2, list(tbad)).any(), route
        assert not np.isnan(d2).any() and (d2 >= 0).all(), route
        for row in qbad:
            assert idx2[row].tolist() == [-1, -1] and d2[row].tolist() == [gc.FLT_MAX, gc.FLT_MAX] and match[row] == -1, \
                (route, row, idx2[row], d2[row], match[row])
        assert same((idx2[good], d2[good], match[good]), (ri[good], rd[good], rm[good])), route
        # the other direction: the special rows as queries and as train rows
        idx2, d2, match = full.swapped().run(route)
        ri, rd, rm = less.swapped().run(route)
        assert not np.isin(idx2, list(qbad)).any(), route
        assert not np.isnan(d2).any() and (d2 >= 0).all(), route
        for row in tbad:
            assert idx2[row].tolist() == [-1, -1] and d2[row].tolist() == [gc.FLT_MAX, gc.FLT_MAX] and match[row] == -1, \
                (route, row, idx2[row], d2[row], match[row])
        # rows of `less` are the kept train rows; a query of qbad among its neighbours is deleted from neither run,
        # so compare the rows whose top-2 in `less` holds no special query
        clean = ~np.isin(ri, list(qbad)).any(1)
        assert clean.mean() > 0.9
        assert same((idx2[keep][clean], d2[keep][clean]), (ri[clean], rd[clean])), route
