"""Batched guided matching on the GPU (sift_hip_match_*_guided_batched / *_epipolar_batched,
sift_hip_project_homography_batched_device; k_match_guided_batch, k_match_epipolar_batch, k_project_homography_batch).

The bar (include/sift_hip.h): pair p of a batched gated call gives, byte for byte, the rows or the records and count of
the single-pair call on that pair -- checked against the numpy rule (tests/guided_batched_cases.py:
sift_amd.cv.guided_top2 / epipolar_top2 / filter_matches / geometry_usable) and against the single-pair device calls
themselves -- and a pair whose nine floats are not usable comes out empty.  F is read from device memory only.
"""
import ctypes

import numpy as np
import pytest

import epipolar_cases as ec
import general_cases as gen
import guided_batched_cases as bc
import guided_cases as gc
import homography_cases as hc

pytestmark = pytest.mark.gpu
INF = float("inf")
GUARD = 64  # canary rows before and after every output
KINDS = ("window", "epipolar")
FILTERS = (dict(), dict(cross_check=False), dict(ratio_both_ways=True, max_distance=30.0))
CAP = 1100  # the largest set of the batch, on either side


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def half(sift, rows):
    return dev(sift, np.asarray(rows).astype(np.float16).view(np.uint16))


class Uploaded:
    """A batch on the device: per pair the fp16 sets and the positions in rows of the given strides (the filler
    columns are NaN), and the geometry records."""

    def __init__(self, sift, pairs, qs=2, ts=2, gstride=52):
        self.pairs, self.qs, self.ts, self.gstride = pairs, qs, ts, gstride
        self.nq, self.nt = [len(p["q"]) for p in pairs], [len(p["t"]) for p in pairs]
        self.q = [half(sift, p["q"]) for p in pairs]
        self.t = [half(sift, p["t"]) for p in pairs]
        self.qxy = [dev(sift, gc.with_stride(p["q_xy"], qs)) for p in pairs]
        self.txy = [dev(sift, gc.with_stride(p["t_xy"], ts)) for p in pairs]
        self.row0 = np.concatenate([[0], np.cumsum(self.nq)]).astype(int)
        self.rows = int(self.row0[-1])
        self.geometry = None
        if "F" in pairs[0]:
            rec = np.full((len(pairs), gstride // 4), 0x7FC00123, np.uint32)
            for i, p in enumerate(pairs):
                rec[i, :9] = np.ascontiguousarray(p["F"]).reshape(-1).view(np.uint32)
            self.geometry = dev(sift, rec)

    def sets(self):
        # an empty set is passed as a null pointer
        return ([d.value if n else 0 for d, n in zip(self.q, self.nq)], self.nq,
                [d.value if n else 0 for d, n in zip(self.t, self.nt)], self.nt)

    def positions(self):
        return [(a.value if n else 0, n, b.value if k else 0, k) for a, n, b, k in zip(self.qxy, self.nq, self.txy, self.nt)]


@pytest.fixture(scope="module")
def uploaded(sift):
    return {kind: Uploaded(sift, bc.batch(kind)) for kind in KINDS}


class Guarded:
    """A device output of `rows` rows of `cols` x `dtype` between GUARD canary rows; every row starts as the canary."""

    def __init__(self, sift, rows, dtype, cols=1):
        self.rows, self.dtype, self.cols = rows, np.dtype(dtype), cols
        self.words = self.dtype.itemsize * cols // 4
        self.d = dev(sift, np.full((rows + 2 * GUARD) * self.words, -77, np.int32))
        self.value = self.d.value + GUARD * self.words * 4

    def read(self):
        """(the rows, whether both guards are intact)."""
        raw = self.d.to_numpy(np.int32, (self.rows + 2 * GUARD, self.words))
        ok = bool(np.all(raw[:GUARD] == -77) and np.all(raw[GUARD + self.rows:] == -77))
        body = raw[GUARD:GUARD + self.rows].copy().reshape(-1).view(self.dtype)
        return (body.reshape(self.rows, self.cols) if self.cols > 1 else body.reshape(self.rows)), ok


def run_top2(sift, m, up, kind, stream=None):
    idx2, d2, mt = Guarded(sift, up.rows, np.int32, 2), Guarded(sift, up.rows, np.float32, 2), Guarded(sift, up.rows, np.int32)
    if kind == "window":
        m.match_guided_batched(*up.sets(), up.positions(), gc.RADIUS, up.qs, up.ts, 0.8, False, idx2.value, d2.value,
                               mt.value, stream)
    else:
        m.match_epipolar_batched(*up.sets(), up.positions(), up.geometry.value, ec.MAX_ERROR, INF, up.gstride, up.qs,
                                 up.ts, 0.8, False, idx2.value, d2.value, mt.value, stream)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    (a, ok_a), (b, ok_b), (c, ok_c) = idx2.read(), d2.read(), mt.read()
    assert ok_a and ok_b and ok_c, "a canary row next to the outputs was written"
    return a.reshape(-1, 2), b.reshape(-1, 2), c.reshape(-1)


def run_lists(sift, m, up, kind, radius=None, **f):
    """Per pair (records up to its count, the rows behind them), and the counts."""
    out, cnt = Guarded(sift, up.rows, sift.DMATCH_DTYPE), Guarded(sift, len(up.pairs), np.int32)
    if kind == "window":
        m.match_list_guided_batched(*up.sets(), up.positions(), gc.RADIUS if radius is None else radius, out.value,
                                    cnt.value, up.qs, up.ts, **f)
    else:
        m.match_list_epipolar_batched(*up.sets(), up.positions(), up.geometry.value, ec.MAX_ERROR, out.value, cnt.value,
                                      INF if radius is None else radius, up.gstride, up.qs, up.ts, **f)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    (rec, ok_r), (counts, ok_c) = out.read(), cnt.read()
    assert ok_r and ok_c, "a canary row next to the outputs was written"
    rec, counts = rec.reshape(-1), counts.reshape(-1)
    lists = []
    for p in range(len(up.pairs)):
        n = int(counts[p])
        assert 0 <= n <= up.nq[p], (p, n)
        rows = rec[up.row0[p]:up.row0[p + 1]]
        assert np.all(rows[n:].view(np.int32) == -77), f"pair {p}: a row past its count was written"
        lists.append(rows[:n])
    return lists, counts


def same(got, ref):
    return len(got) == len(ref) and all(np.asarray(a).dtype == np.asarray(b).dtype and a.shape == b.shape and
                                        a.tobytes() == b.tobytes() for a, b in zip(got, ref))


def single_top2(sift, m, up, kind, p):
    """The single-pair device call on pair p (F from the host, as that call takes it)."""
    nq = up.nq[p]
    idx2, d2, mt = dev(sift, np.full(2 * nq, -77, np.int32)), dev(sift, np.full(2 * nq, -77, np.float32)), \
        dev(sift, np.full(nq, -77, np.int32))
    a = (up.q[p].value, nq, up.t[p].value, up.nt[p], up.qxy[p].value, up.txy[p].value)
    if kind == "window":
        m.match_guided_device(*a, gc.RADIUS, up.qs, up.ts, 0.8, False, idx2.value, d2.value, mt.value)
    else:
        m.match_epipolar_device(*a, up.pairs[p]["F"], ec.MAX_ERROR, INF, up.qs, up.ts, 0.8, False, idx2.value, d2.value,
                                mt.value)
    return idx2.to_numpy(np.int32, (nq, 2)), d2.to_numpy(np.float32, (nq, 2)), mt.to_numpy(np.int32, (nq,))


def single_list(sift, m, up, kind, p, **f):
    nq = up.nq[p]
    out, cnt = dev(sift, np.full(4 * max(nq, 1), -1, np.int32)), dev(sift, np.full(1, -1, np.int32))
    a = (up.q[p].value, nq, up.t[p].value, up.nt[p], up.qxy[p].value, up.txy[p].value)
    if kind == "window":
        m.match_list_guided_device(*a, gc.RADIUS, out.value, cnt.value, up.qs, up.ts, **f)
    else:
        m.match_list_epipolar_device(*a, up.pairs[p]["F"], ec.MAX_ERROR, out.value, cnt.value, INF, up.qs, up.ts, **f)
    return out.to_numpy(sift.DMATCH_DTYPE, (max(nq, 1),))[:int(cnt.to_numpy(np.int32, (1,))[0])]


def usable(pair):
    return pair.get("usable", True)


@pytest.mark.parametrize("kind", KINDS)
def test_top2_is_the_rule_and_the_single_pair_call(sift, uploaded, kind):
    up = uploaded[kind]
    m = sift.Matcher(CAP, CAP, max_pairs=len(up.pairs))
    got = run_top2(sift, m, up, kind)
    want = bc.expected_top2(kind)
    for name, g, w in zip(("idx2", "d2", "match"), got, want):
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert g.tobytes() == w.tobytes(), (kind, name, bad[:8], np.searchsorted(up.row0, bad[:8], "right") - 1)
    for p, pair in enumerate(up.pairs):
        rows = slice(up.row0[p], up.row0[p + 1])
        if not usable(pair):  # the single-pair call refuses these on the host; the batched call empties them
            assert np.all(got[0][rows] == -1) and np.all(got[1][rows] == bc.FLT_MAX) and np.all(got[2][rows] == -1)
            with pytest.raises(sift.SiftHipError):
                single_top2(sift, m, up, kind, p)
            continue
        if up.nq[p] == 0:
            continue
        one = single_top2(sift, m, up, kind, p)
        assert same(one, [g[rows] for g in got]), (kind, p)


@pytest.mark.parametrize("kind", KINDS)
def test_lists_one_pass_and_two(sift, uploaded, kind):
    """Every filter, with max_pairs >= 2 P (both directions in one pass) and max_pairs = P (two passes): the same
    bytes, the numpy rule's, and -- records modulo imgIdx -- the single-pair list calls'."""
    up = uploaded[kind]
    P = len(up.pairs)
    wide, tight = sift.Matcher(CAP, CAP, max_pairs=2 * P), sift.Matcher(CAP, CAP, max_pairs=P)
    for f in FILTERS:
        want = bc.expected_lists(kind, **f)
        for m in (wide, tight):
            lists, counts = run_lists(sift, m, up, kind, **f)
            assert counts.tolist() == [len(w) for w in want], (kind, f)
            assert same(lists, want), (kind, f)
        for p, pair in enumerate(up.pairs):
            if not usable(pair):
                assert counts[p] == 0
    lists, _ = run_lists(sift, wide, up, kind)
    for p, pair in enumerate(up.pairs):
        if usable(pair):
            one = single_list(sift, wide, up, kind, p).copy()
            assert np.all(one["imgIdx"] == 0)
            one["imgIdx"] = p
            assert one.tobytes() == lists[p].tobytes(), (kind, p)


@pytest.mark.parametrize("kind", KINDS)
def test_strides(sift, uploaded, kind):
    """Position strides 3 / 3 and 2 / 3 with NaN filler, geometry records of 36 bytes: the same bytes as 2 / 2 / 52."""
    base = uploaded[kind]
    m = sift.Matcher(CAP, CAP, max_pairs=2 * len(base.pairs))
    want_top2, want = bc.expected_top2(kind), bc.expected_lists(kind)
    for qs, ts, gstride in ((3, 3, 36), (2, 3, 40)):
        up = Uploaded(sift, bc.batch(kind), qs, ts, gstride)
        assert same(run_top2(sift, m, up, kind), want_top2), (qs, ts)
        assert same(run_lists(sift, m, up, kind)[0], want), (qs, ts)
    if kind == "epipolar":
        assert base.geometry.nbytes == 52 * len(base.pairs)
        rec = base.geometry.to_numpy(sift.VERIFY_RESULT_DTYPE, (len(base.pairs),))
        assert rec["F"].tobytes() == b"".join(np.ascontiguousarray(p["F"]).tobytes() for p in base.pairs)


@pytest.mark.parametrize("kind", KINDS)
def test_band_and_window_radius(sift, uploaded, kind):
    """Another radius than the cases were built for (under the epipolar gate: a finite one, the band ANDed with the
    window): pair by pair the numpy rule."""
    from sift_amd import cv

    up = uploaded[kind]
    radius = 40.0
    m = sift.Matcher(CAP, CAP, max_pairs=2 * len(up.pairs))
    lists, _ = run_lists(sift, m, up, kind, radius=radius)
    for p, pair in enumerate(up.pairs):
        a = (pair["q"], pair["t"], pair["q_xy"], pair["t_xy"])
        b = (pair["t"], pair["q"], pair["t_xy"], pair["q_xy"])
        if kind == "window":
            fwd, rev = cv.guided_top2(*a, radius), cv.guided_top2(*b, radius)
        elif usable(pair):
            fwd = cv.epipolar_top2(*a, pair["F"], ec.MAX_ERROR, radius)
            rev = cv.epipolar_top2(*b, pair["F"].T, ec.MAX_ERROR, radius)
        else:
            fwd, rev = bc.nothing(len(pair["q"])), bc.nothing(len(pair["t"]))
        assert lists[p].tobytes() == cv.filter_matches(*fwd, *rev, img_idx=p).tobytes(), (kind, p)


@pytest.mark.parametrize("kind", KINDS)
def test_more_pairs_than_one_launch_holds(sift, uploaded, kind):
    """20 pairs with max_pairs = 40: forward and reverse are one pass of 40 pairs, which is two launches (32 + 8)."""
    src = bc.batch(kind)
    pick = [0, 1, 2, 3] * 5
    up = Uploaded(sift, [src[p] for p in pick])
    m = sift.Matcher(40, 40, max_pairs=40)
    lists, counts = run_lists(sift, m, up, kind)
    ref = bc.expected_lists(kind)
    for i, p in enumerate(pick):
        want = ref[p].copy()
        want["imgIdx"] = i
        assert lists[i].tobytes() == want.tobytes(), (kind, i)
    assert counts[3::4].min() > 0
    top = run_top2(sift, m, up, kind)
    assert top[0].tobytes() == np.concatenate([src[p]["fwd"][0] for p in pick]).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_general_pair_between_integer_pairs(sift, uploaded, kind):
    """A pair of non-integer fp16 rows (tests/general_cases.py, where fp32 rounds) between two integer pairs: its rows
    satisfy the general path's contract under the gate, and its neighbours' bytes are those of the integer batch."""
    c = gen.case("sift_unrounded")
    gate = "window" if kind == "window" else "band"
    src = bc.batch(kind)
    a, b = src[3], src[4]
    mid = dict(q=c.q, t=c.t, q_xy=c.q_xy, t_xy=c.t_xy, F=c.F)
    up = Uploaded(sift, [a, mid, b])
    m = sift.Matcher(CAP, CAP, max_pairs=6)
    idx2 = Guarded(sift, up.rows, np.int32, 2)
    d2 = Guarded(sift, up.rows, np.float32, 2)
    if kind == "window":
        m.match_guided_batched(*up.sets(), up.positions(), gen.RADIUS, 2, 2, 0.8, False, idx2.value, d2.value, 0)
        ref_a, ref_b = (cv_top2(kind, x, gen.RADIUS) for x in (a, b))
    else:
        m.match_epipolar_batched(*up.sets(), up.positions(), up.geometry.value, gen.MAX_ERROR, INF, 52, 2, 2, 0.8, False,
                                 idx2.value, d2.value, 0)
        ref_a, ref_b = a["fwd"], b["fwd"]
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    (gi, ok_i), (gd, ok_d) = idx2.read(), d2.read()
    assert ok_i and ok_d
    gi, gd = gi.reshape(-1, 2), gd.reshape(-1, 2)
    r = up.row0
    assert same((gi[r[0]:r[1]], gd[r[0]:r[1]]), ref_a) and same((gi[r[2]:r[3]], gd[r[2]:r[3]]), ref_b)
    mi, md = gi[r[1]:r[2]], gd[r[1]:r[2]]
    assert np.any(md[mi >= 0] != np.rint(md[mi >= 0]))  # fractional distances: the general path
    gen.check_top2(mi, md, c.fwd.D, c.fwd.B, c.fwd.cand[gate], c.fwd.ref[gate], label=f"batched {kind}")
    # the reverse direction of the same pair, through the list's second half of the pass
    lists, _ = run_lists(sift, m, up, kind, radius=gen.RADIUS if kind == "window" else None, ratio=0.0)
    fwd_ok = np.flatnonzero(mi[:, 0] >= 0)
    assert set(lists[1]["queryIdx"].tolist()) <= set(fwd_ok.tolist()) and len(lists[1]) > 50
    assert np.array_equal(lists[1]["trainIdx"], mi[lists[1]["queryIdx"], 0])


def cv_top2(kind, pair, radius):
    from sift_amd import cv

    assert kind == "window"
    return cv.guided_top2(pair["q"], pair["t"], pair["q_xy"], pair["t_xy"], radius)


@pytest.mark.parametrize("kind", KINDS)
def test_scratch_restored(sift, uploaded, kind):
    """match_device and match_list_device on the same matcher give the same bytes before and after batched gated calls
    with split merges (600 x 1100 has several key groups per pair)."""
    up = uploaded[kind]
    p = bc.SHAPES.index((600, 1100))
    nq, nt = up.nq[p], up.nt[p]
    m = sift.Matcher(CAP, CAP, max_pairs=2 * len(up.pairs))

    def plain():
        idx2, d2 = dev(sift, np.full(2 * nq, -77, np.int32)), dev(sift, np.full(2 * nq, -77, np.float32))
        out, cnt = dev(sift, np.full(4 * nq, -1, np.int32)), dev(sift, np.full(1, -1, np.int32))
        m.match_device(up.q[p].value, nq, up.t[p].value, nt, 0.8, False, idx2.value, d2.value, 0)
        m.match_list_device(up.q[p].value, nq, up.t[p].value, nt, out.value, cnt.value)
        n = int(cnt.to_numpy(np.int32, (1,))[0])
        return (idx2.to_numpy(np.int32, (nq, 2)).tobytes(), d2.to_numpy(np.float32, (nq, 2)).tobytes(), n,
                out.to_numpy(np.int32, (4 * nq,))[:4 * n].tobytes())

    before = plain()
    assert before[2] > 0
    first = run_top2(sift, m, up, kind)
    lists, _ = run_lists(sift, m, up, kind)
    assert plain() == before
    assert same(run_top2(sift, m, up, kind), first) and same(run_lists(sift, m, up, kind)[0], lists)


def test_codes_forms_equal_the_fp16_forms(sift):
    """Three sets as a C5 rank sees them -- packed with multi.pack_codes / code_set, rank 0 against its two peers,
    positions through position_pairs -- under both gates: the records of the fp16 forms on the same sets."""
    import torch

    from sift_amd import multi

    world, n, counts = 3, 320, [300, 257, 320]
    sets, xy = [], []
    for r in range(world):
        q, _, q_xy, _, _ = ec.make_epipolar(n, n, seed=40 + r)
        sets.append(q)
        xy.append(q_xy)
    # rows of rank 0 reappear, noisy, in both peers at the positions the scene gives them
    rng = np.random.default_rng(3)
    for r in (1, 2):
        k = 120
        src, dst = rng.permutation(counts[0])[:k], rng.permutation(counts[r])[:k]
        sets[r][dst] = np.clip(sets[0][src] + rng.integers(-3, 4, (k, 128)), 0, 255)
        a, b = ec.project_pairs(rng, k)
        xy[0][src], xy[r][dst] = a, b
    n_pad = multi.code_block_rows(n)
    dev_rows = [torch.from_numpy(s.astype(np.float16)).cuda() for s in sets]
    blocks = []
    for r in range(world):
        codes, keys = multi.codes_from_rows(dev_rows[r])
        blocks.append(multi.pack_codes(codes, keys, n_pad))
    buf = torch.cat(blocks)
    gathered_xy = torch.from_numpy(np.stack(xy)).cuda().contiguous()
    pairs = multi.code_pairs(counts, 0, world, n_pad)
    pos = multi.position_pairs(gathered_xy, counts, 0, world)
    assert [(p[1], p[3]) for p in pos] == [(p[2], p[5]) for p in pairs] == [(300, 257), (300, 320)]
    F = np.stack([ec.fundamental() * np.float32(s) for s in (3.0, 0.7)])
    dF = dev(sift, F)
    m = sift.Matcher(n, n, max_pairs=4)
    rows = 600
    torch.cuda.synchronize()
    for kind in KINDS:
        got = []
        for codes in (True, False):
            out, cnt = Guarded(sift, rows, sift.DMATCH_DTYPE), Guarded(sift, 2, np.int32)
            q_ptrs, t_ptrs = [dev_rows[0].data_ptr()] * 2, [dev_rows[1].data_ptr(), dev_rows[2].data_ptr()]
            nqs, nts = [300, 300], [257, 320]
            if kind == "window" and codes:
                m.match_list_guided_codes_batched(buf.data_ptr(), buf.data_ptr(), pairs, pos, gen.RADIUS, out.value, cnt.value, 2, 2)
            elif kind == "window":
                m.match_list_guided_batched(q_ptrs, nqs, t_ptrs, nts, pos, gen.RADIUS, out.value, cnt.value, 2, 2)
            elif codes:
                m.match_list_epipolar_codes_batched(buf.data_ptr(), buf.data_ptr(), pairs, pos, dF.value, ec.MAX_ERROR,
                                                    out.value, cnt.value, INF, 36, 2, 2)
            else:
                m.match_list_epipolar_batched(q_ptrs, nqs, t_ptrs, nts, pos, dF.value, ec.MAX_ERROR, out.value, cnt.value,
                                              INF, 36, 2, 2)
            sift._check(sift.lib().sift_hip_device_sync(), "sync")
            (rec, ok_r), (c, ok_c) = out.read(), cnt.read()
            assert ok_r and ok_c
            got.append((rec.tobytes(), c.reshape(-1).tolist()))
        assert got[0] == got[1], kind
        assert min(got[0][1]) > 20, (kind, got[0][1])
        if kind == "epipolar":  # and the numpy rule, pair by pair
            from sift_amd import cv

            rec = np.frombuffer(got[0][0], sift.DMATCH_DTYPE)
            for p, r in enumerate((1, 2)):
                q, t = sets[0][:300], sets[r][:counts[r]]
                fwd = cv.epipolar_top2(q, t, xy[0][:300], xy[r][:counts[r]], F[p], ec.MAX_ERROR)
                rev = cv.epipolar_top2(t, q, xy[r][:counts[r]], xy[0][:300], F[p].T, ec.MAX_ERROR)
                want = cv.filter_matches(*fwd, *rev, img_idx=p)
                assert rec[300 * p:300 * p + got[0][1][p]].tobytes() == want.tobytes(), p


def test_project_homography_batched(sift):
    """P = 3 with different n, one of them 0; a zero H record (all NaN out); one pair in place: per pair
    cv.project_homography's bytes, and nothing next to the outputs is written."""
    from sift_amd import cv

    rng = np.random.default_rng(8)
    H = hc.homography().astype(np.float32)
    Hs = [H, np.zeros((3, 3), np.float32), (H * np.float32(3.0)).astype(np.float32)]
    ns = [300, 0, 1000]
    xys = [(rng.integers(0, 800, (max(n, 1), 2)) * 0.25).astype(np.float32)[:n] for n in ns]
    for stride, gstride in ((3, 52), (2, 36)):
        rec = np.full((3, gstride // 4), 0x7FC00123, np.uint32)
        for i, h in enumerate(Hs):
            rec[i, :9] = h.reshape(-1).view(np.uint32)
        dG = dev(sift, rec)
        dxy = [dev(sift, gc.with_stride(a, stride, 777.0)) for a in xys]
        out0 = Guarded(sift, ns[0], np.float32, 2)
        # set 2 in place (equal strides), set 0 apart into rows of 2 floats: one call per out_stride
        sift.project_homography_batched_device(dG.value, [(dxy[0].value, ns[0], out0.value), (0, 0, 0), (0, 0, 0)], stride,
                                               2, gstride)
        sift.project_homography_batched_device(dG.value, [(0, 0, 0), (0, 0, 0), (dxy[2].value, ns[2], dxy[2].value)],
                                               stride, stride, gstride)
        sift._check(sift.lib().sift_hip_device_sync(), "sync")
        got0, ok = out0.read()
        assert ok and got0.tobytes() == cv.project_homography(Hs[0], xys[0]).tobytes()
        got2 = dxy[2].to_numpy(np.float32, (ns[2], stride))
        assert got2[:, :2].tobytes() == cv.project_homography(Hs[2], xys[2]).tobytes()
        assert stride == 2 or np.all(got2[:, 2] == 777.0)
    # all three in one launch, the zero record between two good ones: its rows are NaN
    ns = [300, 40, 1000]
    xys[1] = (rng.integers(0, 800, (40, 2)) * 0.25).astype(np.float32)
    rec = np.zeros((3, 13), np.uint32)
    for i, h in enumerate(Hs):
        rec[i, :9] = h.reshape(-1).view(np.uint32)
    dG = dev(sift, rec)
    dxy = [dev(sift, gc.with_stride(a, 3)) for a in xys]
    outs = [Guarded(sift, n, np.float32, 2) for n in ns]
    sift.project_homography_batched_device(dG.value, [(d.value, n, o.value) for d, n, o in zip(dxy, ns, outs)], 3, 2)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    for i in range(3):
        got, ok = outs[i].read()
        assert ok and got.tobytes() == cv.project_homography(Hs[i], xys[i]).tobytes(), i
    assert np.isnan(outs[1].read()[0]).all()
    with pytest.raises(sift.SiftHipError):  # a partial overlap inside one set
        sift.project_homography_batched_device(dG.value, [(dxy[0].value, 300, dxy[0].value + 4)], 3, 3)


def chain_pairs(make, shapes):
    out = []
    for i, (nq, nt) in enumerate(shapes):
        q, t, q_xy, t_xy = make(nq, nt, i)
        out.append(dict(q=q, t=t, q_xy=q_xy, t_xy=t_xy))
    return out


def planted_pair(nq, nt, seed, views=hc.plane_pairs):
    """homography_cases.chain_case's recipe with a seed: a planted copy and its query are one scene point in both views
    -- a point of the plane (hc.plane_pairs), or of the two-camera scene (ec.project_pairs).  No decoys, so the
    putative list is mostly the planted pairs."""
    rng = np.random.default_rng(7000 * nq + nt + seed)
    q = rng.integers(0, 128, (nq, 128))
    t = rng.integers(0, 128, (nt, 128))
    k = min(nq, nt) // 2
    src, dst = rng.permutation(nq)[:k], rng.permutation(nt)[:k]
    amp = rng.integers(2, 9, k)
    t[dst] = np.clip(q[src] + rng.integers(-amp[:, None], amp[:, None] + 1, (k, 128)), 0, 255)
    q_xy = rng.integers(0, int(4 * ec.SIDE), (nq, 2)) * 0.25
    t_xy = rng.integers(0, int(4 * ec.SIDE), (nt, 2)) * 0.25
    q_xy[src], t_xy[dst] = views(rng, k)
    return q.astype(np.float32), t.astype(np.float32), q_xy.astype(np.float32), t_xy.astype(np.float32)


CHAIN_SHAPES = [(400, 380), (300, 330), (6, 5)]  # the last pair's list is too short for either model


def putative_lists(pairs):
    from sift_amd import cv

    out = []
    for p in pairs:
        every = np.ones((len(p["q"]), len(p["t"])), bool)
        fwd, rev = cv.mask_top2(p["q"], p["t"], every), cv.mask_top2(p["t"], p["q"], every.T)
        out.append(cv.filter_matches(*fwd, *rev))
    return out


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_chain_on_one_stream(sift, model):
    """match_list_batched -> verify_*_batched_device -> (project_homography_batched_device ->) the batched guided
    rematch with the geometry read from the verifier's records, on one stream with no read-back until the end: every
    stage equals the numpy chain of its pair with the seed + p; the pair with too few matches gets an empty list."""
    import torch

    from sift_amd import cv

    K, seed, radius = 256, 5, 2.0
    homography = model == "homography"
    make = planted_pair if homography else (lambda nq, nt, s: planted_pair(nq, nt, s, ec.project_pairs))
    pairs = chain_pairs(make, CHAIN_SHAPES)
    up = Uploaded(sift, pairs, 3, 3)
    P = len(pairs)
    rows = up.rows
    m, v = sift.Matcher(400, 400, max_pairs=2 * P), sift.Verifier(rows, K, P)
    lst, cnt = Guarded(sift, rows, sift.DMATCH_DTYPE), Guarded(sift, P, np.int32)
    res = Guarded(sift, P, sift.VERIFY_RESULT_DTYPE)
    proj = [Guarded(sift, n, np.float32, 2) for n in up.nq]
    out2, cnt2 = Guarded(sift, rows, sift.DMATCH_DTYPE), Guarded(sift, P, np.int32)
    # the matcher's first list call allocates its select scratch: once, outside the chain
    warm, wcnt = dev(sift, np.zeros(16 * rows, np.uint8)), dev(sift, np.zeros(4 * P, np.uint8))
    m.match_list_batched(*up.sets(), warm.value, wcnt.value)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    vpairs = [(a, n, b, k, n) for a, n, b, k in up.positions()]
    s = torch.cuda.Stream()
    st = s.cuda_stream
    m.match_list_batched(*up.sets(), lst.value, cnt.value, stream=st)
    if homography:
        v.verify_homography_batched_device(lst.value, cnt.value, vpairs, res.value, 0, 0, 0, hc.MAX_ERROR, K, seed, 3, 3,
                                           stream=st)
        sift.project_homography_batched_device(res.value, [(a.value, n, o.value) for a, n, o in zip(up.qxy, up.nq, proj)],
                                               3, 2, 52, stream=st)
        pos = [(o.value, n, b.value, k) for o, n, b, k in zip(proj, up.nq, up.txy, up.nt)]
        # strides differ per side: the projected rows have 2 floats, the train rows 3
        m.match_list_guided_batched(*up.sets(), pos, radius, out2.value, cnt2.value, 2, 3, stream=st)
    else:
        v.verify_batched_device(lst.value, cnt.value, vpairs, res.value, 0, 0, 0, ec.MAX_ERROR, K, seed, 3, 3, stream=st)
        m.match_list_epipolar_batched(*up.sets(), up.positions(), res.value, ec.MAX_ERROR, out2.value, cnt2.value, INF, 52,
                                      3, 3, stream=st)
    s.synchronize()
    (rec, ok1), (n1, ok2), (r, ok3), (rec2, ok4), (n2, ok5) = lst.read(), cnt.read(), res.read(), out2.read(), cnt2.read()
    assert ok1 and ok2 and ok3 and ok4 and ok5
    rec, rec2, n1, n2, r = rec.reshape(-1), rec2.reshape(-1), n1.reshape(-1), n2.reshape(-1), r.reshape(-1)
    putative = putative_lists(pairs)
    short = P - 1
    assert len(putative[short]) < (4 if homography else 8) and min(len(x) for x in putative[:short]) >= 100
    for p, pair in enumerate(pairs):
        want1 = putative[p].copy()
        want1["imgIdx"] = p
        assert n1[p] == len(want1) and rec[up.row0[p]:up.row0[p] + n1[p]].tobytes() == want1.tobytes(), p
        if homography:
            ref = cv.ransac_homography(putative[p], pair["q_xy"], pair["t_xy"], hc.MAX_ERROR, K, seed + p)
            G = ref["H"]
        else:
            ref = cv.ransac_fundamental(putative[p], pair["q_xy"], pair["t_xy"], ec.MAX_ERROR, K, seed + p)
            G = ref["F"]
        G = np.asarray(G, np.float32).reshape(3, 3)
        assert r[p]["F"].tobytes() == G.tobytes() and r[p]["hypothesis"] == ref["hypothesis"], p
        assert (ref["hypothesis"] < 0) == (p == short)
        a = (pair["q"], pair["t"], pair["q_xy"], pair["t_xy"])
        b = (pair["t"], pair["q"], pair["t_xy"], pair["q_xy"])
        if homography:
            want_proj = cv.project_homography(G, pair["q_xy"])
            got_proj, okp = proj[p].read()
            assert okp and got_proj.tobytes() == want_proj.tobytes(), p
            fwd = cv.guided_top2(pair["q"], pair["t"], want_proj, pair["t_xy"], radius)
            rev = cv.guided_top2(pair["t"], pair["q"], pair["t_xy"], want_proj, radius)
        elif cv.geometry_usable(G):
            fwd, rev = cv.epipolar_top2(*a, G, ec.MAX_ERROR), cv.epipolar_top2(*b, G.T, ec.MAX_ERROR)
        else:
            fwd, rev = bc.nothing(len(pair["q"])), bc.nothing(len(pair["t"]))
        want2 = cv.filter_matches(*fwd, *rev, img_idx=p)
        assert n2[p] == len(want2) and rec2[up.row0[p]:up.row0[p] + n2[p]].tobytes() == want2.tobytes(), p
        assert np.all(rec2[up.row0[p] + n2[p]:up.row0[p + 1]].view(np.int32) == -77)
        assert (len(want2) == 0) == (p == short), (p, len(want2))


def test_host_conveniences(sift):
    """matchListGuidedBatched / matchListEpipolarBatched on host arrays: the reference lists."""
    pairs = bc.batch("epipolar")
    pick = [3, 4, 9]  # two usable pairs and the zero record
    desc = [(pairs[p]["q"], pairs[p]["t"]) for p in pick]
    xy = [(pairs[p]["q_xy"], pairs[p]["t_xy"]) for p in pick]
    got = sift.matchListEpipolarBatched(desc, xy, [pairs[p]["F"] for p in pick], ec.MAX_ERROR)
    ref = bc.expected_lists("epipolar")
    for i, p in enumerate(pick):
        want = ref[p].copy()
        want["imgIdx"] = i
        assert got[i].tobytes() == want.tobytes(), p
    assert len(got[2]) == 0 and len(got[0]) > 0
    wp = bc.batch("window")
    got = sift.matchListGuidedBatched([(wp[p]["q"], wp[p]["t"]) for p in (4, 7, 3)],
                                      [(wp[p]["q_xy"], wp[p]["t_xy"]) for p in (4, 7, 3)], gc.RADIUS, cross_check=False)
    ref = bc.expected_lists("window", cross_check=False)
    for i, p in enumerate((4, 7, 3)):
        want = ref[p].copy()
        want["imgIdx"] = i
        assert got[i].tobytes() == want.tobytes(), p


def test_argument_errors_launch_nothing(sift, uploaded):
    """The rules that need a matcher: P outside 1..max_pairs, sizes over the limits (the reverse direction's too), null
    descriptor or position pointers of non-empty sets.  Nothing is written, and the matcher stays usable."""
    up = uploaded["epipolar"]
    L = sift.lib()
    P = 4
    m = sift.Matcher(300, 40, max_pairs=P)
    out, cnt = Guarded(sift, 400, sift.DMATCH_DTYPE), Guarded(sift, P, np.int32)
    f = sift._match_filter(cross_check=False)

    def call(pick, flt=f, q_null=None, xy_null=None, P_arg=None, pairs=True):
        n = len(pick)
        qa = (ctypes.c_void_p * n)(*[None if i == q_null else up.q[p].value for i, p in enumerate(pick)])
        ta = (ctypes.c_void_p * n)(*[up.t[p].value for p in pick])
        na, ma = (ctypes.c_int * n)(*[up.nq[p] for p in pick]), (ctypes.c_int * n)(*[up.nt[p] for p in pick])
        pos = (sift._MatchPositions * n)(*[sift._MatchPositions(up.qxy[p].value, None if i == xy_null else up.txy[p].value)
                                           for i, p in enumerate(pick)])
        rc = L.sift_hip_match_list_epipolar_batched(m._m, n if P_arg is None else P_arg, qa, na, ta, ma,
                                                    pos if pairs else None, 2, 2, INF, up.geometry.value, 52,
                                                    ec.MAX_ERROR, ctypes.byref(flt), out.value, cnt.value, None)
        return rc, L.sift_hip_last_error().decode()

    small = [0, 1, 3]  # (1, 1), (1, 40), (33, 31)
    for kw, word in ((dict(pick=small, P_arg=0), "bad gated batch"), (dict(pick=small + small), "bad gated batch"),
                     (dict(pick=small, pairs=False), "bad gated batch"),
                     (dict(pick=[0, 4]), "pair size exceeds matcher limits"),  # 257 x 300: nt over max_train
                     (dict(pick=small, q_null=2), "null descriptor pointer"),
                     (dict(pick=small, xy_null=1), "epipolar gate: null position pointer")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    # the reverse pair of a cross-checked list does not fit this matcher (max_query 40 >= 31, but max_train 31 < 33)
    tight = sift.Matcher(40, 31, max_pairs=2)
    sets = ([up.q[3].value], [33], [up.t[3].value], [31])
    with pytest.raises(sift.SiftHipError, match="reverse pair"):
        tight.match_list_epipolar_batched(*sets, [(up.qxy[3].value, up.txy[3].value)], up.geometry.value, ec.MAX_ERROR,
                                          out.value, cnt.value, INF, 52, 2, 2)
    sift._check(L.sift_hip_device_sync(), "sync")
    assert np.all(out.read()[0].view(np.int32) == -77) and np.all(cnt.read()[0] == -77)
    tight.match_list_epipolar_batched(*sets, [(up.qxy[3].value, up.txy[3].value)], up.geometry.value + 3 * 52,
                                      ec.MAX_ERROR, out.value, cnt.value, INF, 52, 2, 2, cross_check=False)
    sift._check(L.sift_hip_device_sync(), "sync")
    want = bc.expected_lists("epipolar", cross_check=False)[3].copy()
    want["imgIdx"] = 0
    n = int(cnt.read()[0].reshape(-1)[0])
    assert n == len(want) and out.read()[0].reshape(-1)[:n].tobytes() == want.tobytes()
