"""The relative pose from a verified homography on the GPU (sift_hip_recover_pose_homography_*; kernels in
csrc/pose_homography.hip).

The bar: the 96-byte plane pose record, the four 64-byte candidates, the in-front mask, the points (NaN bit patterns
included), the in-front records and their count equal sift_amd.cv.recover_pose_homography (the rule of
include/sift_hip.h in numpy float64) as raw bytes, in the single-pair and the batched form, and nothing else is
written.  The inputs are tests/plane_pose_cases.py; tests/test_plane_pose_cases.py checks the mirror itself on the CPU.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import plane_pose_cases as pc
import pose_cases as fc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs, and the bytes no call may touch, start as this byte
GUARD = 96
NAN_BITS = 0x7FC00000
U, T = pc.UNIQUE_SEEDS, pc.TIED_SEEDS
OPTIONAL = ("mask_out", "points", "out", "out_count", "candidates")


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def sync(sift):
    sift._check(sift.lib().sift_hip_device_sync(), "sync")


def record(sift, result):
    r = np.zeros(1, sift.HOMOGRAPHY_RESULT_DTYPE)
    r["H"][0] = result["H"]
    r["hypothesis"][0] = result["hypothesis"]
    return r


def rule(s, n=None, mask=None, result=None, **kw):
    """cv.recover_pose_homography on the first n records of a scene."""
    from sift_amd import cv

    n = len(s["matches"]) if n is None else n
    mask = s["mask"] if mask is None else mask
    return cv.recover_pose_homography(s["matches"][:n], s["q_xy"], s["t_xy"], result or s["result"], mask[:n], s["cam_q"],
                                      s["cam_t"], **kw)


def pose(sift, s, count=None, stride=(2, 2), v=None, mask=None, result=None, alias=False, skip=(), stream=None, **kw):
    """recover_pose_homography_device on an uploaded scene; everything it may write, back on the host.  skip: the
    optional outputs passed as null; alias: mask_out is the mask."""
    buf = s["matches"]
    cap = len(buf)
    v = v or sift.Verifier(max(cap, 1), 1)
    dm = dev(sift, buf) if cap else None
    dq, dt = dev(sift, ec.with_stride(s["q_xy"], stride[0])), dev(sift, ec.with_stride(s["t_xy"], stride[1]))
    dc = dev(sift, np.int32([count])) if count is not None else None
    mask0 = np.full(cap + GUARD, FILL, np.uint8)
    mask0[:cap] = s["mask"] if mask is None else mask
    res, dmask = dev(sift, record(sift, result or s["result"])), dev(sift, mask0)
    o = dict(pose=dev(sift, np.full(96 + GUARD, FILL, np.uint8)), mask_out=dev(sift, np.full(cap + GUARD, FILL, np.uint8)),
             points=dev(sift, np.full(12 * (cap + GUARD), FILL, np.uint8)),
             out=dev(sift, np.full(16 * (cap + GUARD), FILL, np.uint8)), out_count=dev(sift, np.full(4 + GUARD, FILL, np.uint8)),
             candidates=dev(sift, np.full(256 + GUARD, FILL, np.uint8)))
    ptr = {k: (0 if k in skip else a.value) for k, a in o.items()}
    if alias:
        ptr["mask_out"] = dmask.value
    v.recover_pose_homography_device(dm.value if dm else 0, dc.value if dc else 0, cap, dq.value, len(s["q_xy"]), dt.value,
                                     len(s["t_xy"]), res.value, dmask.value, s["cam_q"], s["cam_t"], ptr["pose"],
                                     ptr["mask_out"], ptr["points"], ptr["out"], ptr["out_count"], ptr["candidates"],
                                     q_stride=stride[0], t_stride=stride[1],
                                     stream=stream.cuda_stream if stream else None, **kw)
    if stream:
        stream.synchronize()
    else:
        sync(sift)
    return dict(pose=o["pose"].to_numpy(np.uint8, (96 + GUARD,)), mask_out=o["mask_out"].to_numpy(np.uint8, (cap + GUARD,)),
                points=o["points"].to_numpy(np.uint32, (cap + GUARD, 3)), out=o["out"].to_numpy(sift.DMATCH_DTYPE, (cap + GUARD,)),
                out_count=o["out_count"].to_numpy(np.uint8, (4 + GUARD,)),
                candidates=o["candidates"].to_numpy(np.uint8, (256 + GUARD,)), mask=dmask.to_numpy(np.uint8, (cap + GUARD,)),
                result=res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,)))


def check(got, ref, buf, n, skip=(), alias=False):
    """Every output of a plane pose call against the numpy rule's dict for the n records that count."""
    cap = len(buf)
    assert got["pose"][:96].tobytes() == pc.plane_pose_bytes(ref), (got["pose"][:96].view(np.int32), ref)
    assert (got["pose"][96:] == FILL).all()
    if "candidates" in skip:
        assert (got["candidates"] == FILL).all()
    else:
        assert got["candidates"][:256].tobytes() == ref["candidates"].tobytes(), (got["candidates"][:256].view(np.float32),
                                                                                 ref["candidates"])
        assert (got["candidates"][256:] == FILL).all()
    want_mask = np.zeros(cap, np.uint8)
    want_mask[:n] = ref["mask"]
    side = got["mask"] if alias else got["mask_out"]
    if "mask_out" in skip:
        assert (got["mask_out"] == FILL).all()
    else:
        assert np.array_equal(side[:cap], want_mask) and (side[cap:] == FILL).all()  # bytes in [n, cap) are zero
    if "points" in skip:
        assert (got["points"].view(np.uint8) == FILL).all()
    else:
        assert got["points"][:n].tobytes() == ref["points"].view(np.uint32).tobytes()
        assert (got["points"][:n][ref["mask"] == 0] == NAN_BITS).all()
        assert (got["points"][n:].view(np.uint8) == FILL).all()  # rows at and past n are not written
    k = len(ref["list"])
    if "out" in skip:
        assert (got["out"].view(np.uint8) == FILL).all()
    else:
        assert got["out"][:k].tobytes() == ref["list"].tobytes() == buf[:n][ref["mask"] != 0].tobytes()
        assert (got["out"][k:].view(np.uint8) == FILL).all()
    if "out_count" in skip:
        assert (got["out_count"] == FILL).all()
    else:
        assert got["out_count"][:4].view(np.int32)[0] == k == ref["in_front"] and (got["out_count"][4:] == FILL).all()


def the_inputs_stay(sift, got, s, alias=False):
    assert got["result"].tobytes() == record(sift, s["result"]).tobytes()
    if not alias:
        assert np.array_equal(got["mask"][:len(s["mask"])], s["mask"]) and (got["mask"][len(s["mask"]):] == FILL).all()


# every shape with the planted records marked, and with the unrelated ones marked too ("mask_all both ways")
SHAPES = [(s, a) for s in pc.SHAPES if s != (0, 0) for a in (False, True)]


@pytest.mark.parametrize("shape,mask_all", SHAPES, ids=["%d+%d-%s" % (s[0], s[1], "all" if a else "planted") for s, a in SHAPES])
def test_shapes(sift, shape, mask_all):
    s = pc.scene(U[0], shape[0], shape[1], mask_all)
    ref = pc.reference(U[0], shape[0], shape[1], mask_all)
    got = pose(sift, s)
    print(shape, "fit", ref["fit"], "counts", ref["counts"], "candidate", ref["candidate"], "parallax", ref["with_parallax"])
    check(got, ref, s["matches"], len(s["matches"]))
    the_inputs_stay(sift, got, s)
    assert ref["candidate"] >= 0 and ref["in_front"] >= shape[0]


@pytest.mark.parametrize("mask_all", [False, True])
def test_the_empty_shape(sift, mask_all):
    """(0, 0) of SHAPES: no record; the position arrays hold one unused row so that their pointers are not null."""
    s = dict(pc.scene(U[0], 0, 0, mask_all))
    s["q_xy"], s["t_xy"] = np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32)
    ref = rule(s)
    assert ref["candidate"] == -1 and ref["fit"] == 0 and ref["candidates"].view(np.uint8).any()
    check(pose(sift, s), ref, s["matches"], 0)


def test_empty_list_with_cap_0(sift):
    s = pc.scene(U[0], 4)
    v = sift.Verifier(1, 1)
    res = dev(sift, record(sift, s["result"]))
    out = dev(sift, np.full(96 + GUARD, FILL, np.uint8))
    cnt = dev(sift, np.full(4, FILL, np.uint8))
    cands = dev(sift, np.full(256 + GUARD, FILL, np.uint8))
    v.recover_pose_homography_device(0, 0, 0, 0, 0, 0, 0, res.value, 0, s["cam_q"], s["cam_t"], out.value, 0, 0, 0, cnt.value,
                                     cands.value)
    sync(sift)
    got, ref = out.to_numpy(np.uint8, (96 + GUARD,)), rule(s, 0)
    assert got[:96].tobytes() == pc.plane_pose_bytes(ref) and (got[96:] == FILL).all()
    assert got[:96].view(np.int32)[18] == -1 and cnt.to_numpy(np.int32, (1,))[0] == 0
    c = cands.to_numpy(np.uint8, (256 + GUARD,))
    assert c[:256].tobytes() == ref["candidates"].tobytes() and c[:256].any() and (c[256:] == FILL).all()


@pytest.mark.parametrize("count", [200, 0, 360, 1000, -3])
def test_a_device_count_below_and_past_cap(sift, count):
    s = pc.scene(U[0], 300, 60, True)
    n = min(max(count, 0), 360)
    got = pose(sift, s, count=count)
    check(got, rule(s, n), s["matches"], n)


@pytest.mark.parametrize("strides", [(3, 3), (5, 2)])
def test_strides_give_identical_results(sift, strides):
    s = pc.scene(U[1], 300, 60, True)
    got = pose(sift, s, stride=strides)
    check(got, pc.reference(U[1], 300, 60, True), s["matches"], 360)
    assert all(got[k].tobytes() == b.tobytes() for k, b in pose(sift, s).items())


def test_mask_out_may_be_the_mask(sift):
    s = pc.scene(U[0], 1100, 100, True)
    ref = pc.reference(U[0], 1100, 100, True)
    assert 0 < ref["in_front"] < 1200  # the call changes the mask
    got = pose(sift, s, alias=True)
    check(got, ref, s["matches"], 1200, skip=("mask_out",), alias=True)
    assert np.array_equal(got["mask"][:1200], ref["mask"])
    got = pose(sift, s, alias=True, count=700)  # the rows in [n, cap) of the mask become 0
    check(got, rule(s, 700), s["matches"], 700, skip=("mask_out",), alias=True)
    assert not got["mask"][700:1200].any()


@pytest.mark.parametrize("skip", [(k,) for k in OPTIONAL] + [OPTIONAL], ids=lambda s: "+".join(s))
def test_each_optional_output_may_be_null(sift, skip):
    s = pc.scene(U[2], 300, 60, True)
    check(pose(sift, s, skip=skip), pc.reference(U[2], 300, 60, True), s["matches"], 360, skip=skip)


def test_thresholds(sift):
    seed = U[0]
    s = pc.scene(seed, 300, 60, True)
    full = pc.reference(seed, 300, 60, True)
    far = pc.reference(seed, 300, 60, True, float("inf"))
    check(pose(sift, s, max_depth=float("inf")), far, s["matches"], 360)
    assert far["in_front"] >= full["in_front"]
    depth = float(np.sort(full["points"][full["mask"] != 0, 2])[full["in_front"] // 2])
    near = pc.reference(seed, 300, 60, True, depth)
    assert 0 < near["in_front"] < full["in_front"]
    check(pose(sift, s, max_depth=depth), near, s["matches"], 360)
    # a bar between the two extremes that splits the set: found by bisection on the rule
    lo, hi = -1.0, 1.0
    for _ in range(40):
        bar = float(np.float32((lo + hi) / 2))
        k = pc.reference(seed, 300, 60, True, 50.0, bar)["with_parallax"]
        if 0 < k < full["in_front"]:
            break
        lo, hi = (bar, hi) if k == 0 else (lo, bar)
    tight = pc.reference(seed, 300, 60, True, 50.0, bar)
    assert 0 < tight["with_parallax"] < full["in_front"]
    check(pose(sift, s, max_cos_parallax=bar), tight, s["matches"], 360)
    for bar in (-1.0, 1.0):
        check(pose(sift, s, max_cos_parallax=bar), pc.reference(seed, 300, 60, True, 50.0, bar), s["matches"], 360)


def test_all_four_candidates_win(sift):
    winners = set()
    for seed in U:
        s, ref = pc.scene(seed), pc.reference(seed)
        check(pose(sift, s), ref, s["matches"], pc.DRAWN)
        winners.add(int(ref["candidate"]))
    assert winners == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", T)
def test_tied_scenes(sift, seed):
    s, ref = pc.scene(seed), pc.reference(seed)
    got = pose(sift, s)
    check(got, ref, s["matches"], pc.DRAWN)
    counts = got["pose"][56:72].view(np.int32)
    assert sorted(counts)[-2:] == [pc.DRAWN, pc.DRAWN] and int(got["pose"][72:76].view(np.int32)[0]) == int(np.argmax(counts))


def test_degenerate_inputs_give_the_empty_result(sift):
    s = pc.scene(U[0])
    n = len(s["matches"])
    bad = s["H"].copy()
    bad[4] = np.nan
    inf = s["H"].copy()
    inf[0] = np.inf
    nan_w = s["H"].copy()
    nan_w[8] = np.nan
    for result, fit in (({"H": s["H"], "hypothesis": -1}, n), ({"H": np.zeros(9, np.float32), "hypothesis": 0}, 0),
                        ({"H": bad, "hypothesis": 0}, n), ({"H": inf, "hypothesis": 0}, n), ({"H": nan_w, "hypothesis": 0}, 0),
                        ({"H": pc.RANK1, "hypothesis": 0}, n), ({"H": -s["H"], "hypothesis": 0}, 0)):
        ref = rule(s, result=result)
        assert ref["candidate"] == -1 and ref["fit"] == fit
        check(pose(sift, s, result=result), ref, s["matches"], n)
    zeros = np.zeros(n, np.uint8)
    ref = rule(s, mask=zeros)
    assert ref["candidate"] == -1 and ref["fit"] == 0
    check(pose(sift, s, mask=zeros), ref, s["matches"], n)
    # masked records with NaN positions or indices outside the arrays are no fit records
    t = dict(s)
    t["q_xy"] = s["q_xy"].copy()
    t["q_xy"][:5] = np.nan
    t["matches"] = s["matches"].copy()
    t["matches"]["trainIdx"][5:9] = n + 7
    t["matches"]["queryIdx"][9:11] = -1
    ref = rule(t)
    assert ref["fit"] == n - 11 == ref["in_front"]
    check(pose(sift, t), ref, t["matches"], n)
    t["q_xy"][:] = np.nan
    ref = rule(t)
    assert ref["candidate"] == -1 and ref["fit"] == 0
    check(pose(sift, t), ref, t["matches"], n)


def test_a_pure_rotation(sift):
    """H = Kt R Kq^-1: the decomposition exists, with a distance past 1e4 (tests/test_plane_pose_cases.py)."""
    s = dict(pc.scene(U[0]))
    Kq, Kt = pc.kmat(s["cam_q"]), pc.kmat(s["cam_t"])
    H = Kt @ s["R"] @ np.linalg.inv(Kq)
    H = (H / np.linalg.norm(H)).astype(np.float32).reshape(9)
    rays = np.concatenate([s["q_xy"].astype(np.float64), np.ones((pc.DRAWN, 1))], 1) @ np.linalg.inv(Kq).T @ s["R"].T @ Kt.T
    s["t_xy"] = (rays[:, :2] / rays[:, 2:]).astype(np.float32)
    s["matches"] = s["matches"].copy()
    s["matches"]["trainIdx"] = s["matches"]["queryIdx"]
    result = {"H": H, "hypothesis": 0}
    ref = rule(s, result=result)
    assert (ref["candidates"]["distance"] > 1e4).all()
    check(pose(sift, s, result=result), ref, s["matches"], pc.DRAWN)


def test_two_runs_and_another_stream_give_the_same_bytes(sift):
    import torch

    s = pc.scene(U[3], 1100, 100, True)
    v = sift.Verifier(1200, 1)
    a = pose(sift, s, v=v)
    check(a, pc.reference(U[3], 1100, 100, True), s["matches"], 1200)
    b = pose(sift, s, v=v)
    c = pose(sift, s, v=v, stream=torch.cuda.Stream())
    assert all(a[k].tobytes() == b[k].tobytes() == c[k].tobytes() for k in a)


class Batch:
    """Scenes as the pairs of one batched call: ragged caps, a device count per pair, per-pair cameras and records."""

    def __init__(self, sift, items, stride=(2, 2)):
        """items: (scene, count or None, result or None) per pair; a scene of None is a pair with cap 0."""
        self.sift, self.stride = sift, stride
        first = next(s for s, _, _ in items if s is not None)
        self.scenes = [s for s, _, _ in items]
        self.caps = [len(s["matches"]) if s else 0 for s in self.scenes]
        self.n = [cap if c is None else min(max(c, 0), cap) for (_, c, _), cap in zip(items, self.caps)]
        self.results = [(r or s["result"]) if s else first["result"] for s, _, r in items]
        self.row0 = np.concatenate([[0], np.cumsum(self.caps)]).astype(int)
        self.P, self.rows = len(items), int(self.row0[-1])
        self.dm = dev(sift, np.concatenate([s["matches"] for s in self.scenes if s]))
        self.dc = dev(sift, np.int32([cap if c is None else c for (_, c, _), cap in zip(items, self.caps)]))
        self.dxy = [(dev(sift, ec.with_stride(s["q_xy"], stride[0])), dev(sift, ec.with_stride(s["t_xy"], stride[1])))
                    if s else None for s in self.scenes]
        self.pairs = [(d[0].value, len(s["q_xy"]), d[1].value, len(s["t_xy"]), cap) if s else (0, 0, 0, 0, 0)
                      for s, d, cap in zip(self.scenes, self.dxy, self.caps)]
        self.cams_q = np.stack([(s or first)["cam_q"] for s in self.scenes])
        self.cams_t = np.stack([(s or first)["cam_t"] for s in self.scenes])
        self.mask0 = np.full(self.rows + GUARD, FILL, np.uint8)
        for p, s in enumerate(self.scenes):
            if s:
                self.mask0[self.row0[p]: self.row0[p + 1]] = s["mask"]
        self.res0 = np.concatenate([record(sift, r) for r in self.results])
        self.dres, self.dmask = dev(sift, self.res0), dev(sift, self.mask0)

    def outputs(self):
        s = self.sift
        return dict(pose=dev(s, np.full(96 * (self.P + 1), FILL, np.uint8)),
                    mask_out=dev(s, np.full(self.rows + GUARD, FILL, np.uint8)),
                    points=dev(s, np.full(12 * (self.rows + GUARD), FILL, np.uint8)),
                    out=dev(s, np.full(16 * (self.rows + GUARD), FILL, np.uint8)),
                    out_count=dev(s, np.full(4 * (self.P + 1), FILL, np.uint8)),
                    candidates=dev(s, np.full(256 * (self.P + 1), FILL, np.uint8)))

    def read(self, o):
        s = self.sift
        return dict(pose=o["pose"].to_numpy(np.uint8, (self.P + 1, 96)), mask_out=o["mask_out"].to_numpy(np.uint8, (self.rows + GUARD,)),
                    points=o["points"].to_numpy(np.uint32, (self.rows + GUARD, 3)),
                    out=o["out"].to_numpy(s.DMATCH_DTYPE, (self.rows + GUARD,)),
                    out_count=o["out_count"].to_numpy(np.int32, (self.P + 1,)),
                    candidates=o["candidates"].to_numpy(np.uint8, (self.P + 1, 256)),
                    mask=self.dmask.to_numpy(np.uint8, (self.rows + GUARD,)), result=self.dres.to_numpy(np.uint8, (52 * self.P,)))

    def run(self, v, stream=None, o=None, **kw):
        o = o or self.outputs()
        v.recover_pose_homography_batched_device(self.dm.value, self.dc.value, self.pairs, self.dres.value, self.dmask.value,
                                                 self.cams_q, self.cams_t, o["pose"].value, o["mask_out"].value,
                                                 o["points"].value, o["out"].value, o["out_count"].value,
                                                 o["candidates"].value, q_stride=self.stride[0], t_stride=self.stride[1],
                                                 stream=stream.cuda_stream if stream else None, **kw)
        if stream:
            stream.synchronize()
        else:
            sync(self.sift)
        return self.read(o)

    def singles(self, v):
        """The same pairs through P single-pair calls on the same verifier, laid out as the batch."""
        o = self.outputs()
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            a = int(self.row0[p])
            v.recover_pose_homography_device(self.dm.value + 16 * a if cap else 0, self.dc.value + 4 * p, cap, q, nq, t, nt,
                                             self.dres.value + 52 * p, self.dmask.value + a if cap else 0, self.cams_q[p],
                                             self.cams_t[p], o["pose"].value + 96 * p, o["mask_out"].value + a,
                                             o["points"].value + 12 * a, o["out"].value + 16 * a, o["out_count"].value + 4 * p,
                                             o["candidates"].value + 256 * p, q_stride=self.stride[0], t_stride=self.stride[1])
        sync(self.sift)
        return self.read(o)

    def check(self, got):
        for p, s in enumerate(self.scenes):
            a, cap, n = int(self.row0[p]), self.caps[p], self.n[p]
            if s is None:
                assert got["pose"][p, 72:80].view(np.int32).tolist() == [-1, 0] and got["out_count"][p] == 0, p
                continue
            ref = rule(s, n, result=self.results[p])
            assert got["pose"][p].tobytes() == pc.plane_pose_bytes(ref), p
            assert got["candidates"][p].tobytes() == ref["candidates"].tobytes(), p
            mask = got["mask_out"][a:a + cap]
            assert np.array_equal(mask[:n], ref["mask"]) and not mask[n:].any(), p
            pts = got["points"][a:a + cap]
            assert pts[:n].tobytes() == ref["points"].view(np.uint32).tobytes(), p
            assert (pts[n:].view(np.uint8) == FILL).all(), p
            k = len(ref["list"])
            rows = got["out"][a:a + cap]
            assert got["out_count"][p] == k and rows[:k].tobytes() == ref["list"].tobytes(), p
            assert (rows[k:].view(np.uint8) == FILL).all(), p
        assert (got["pose"][self.P:] == FILL).all() and (got["out_count"][self.P:].view(np.uint8) == FILL).all()
        assert (got["candidates"][self.P:] == FILL).all()
        for key in ("mask_out", "points", "out"):
            assert (got[key][self.rows:].view(np.uint8) == FILL).all(), key
        assert got["mask"].tobytes() == self.mask0.tobytes() and got["result"].tobytes() == self.res0.tobytes()


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def mixed(sift, stride=(2, 2)):
    """P = 5: ragged caps, different cameras per pair, an empty record, a tied scene, a count below cap."""
    return Batch(sift, [(pc.scene(U[0], 300, 60, True), None, None), (pc.scene(U[1], 63), None, None),
                        (pc.scene(U[2], 64, 1), None, {"H": pc.scene(U[2])["H"], "hypothesis": -1}),
                        (pc.scene(T[0]), None, None), (pc.scene(U[4], 1100, 100, True), 901, None)], stride)


@pytest.fixture(scope="module")
def verifier(sift):
    return sift.Verifier(64 * 72, 1, 64)


def test_mixed_batch_equals_the_rule_and_the_single_calls(sift, verifier):
    b = mixed(sift)
    got = b.run(verifier)
    b.check(got)
    assert int(got["pose"][2, 72:76].view(np.int32)[0]) == -1
    counts = got["pose"][3, 56:72].view(np.int32)
    assert sorted(counts)[-2:] == [pc.DRAWN, pc.DRAWN]  # the tied pair
    assert len({b.cams_q[p].tobytes() for p in range(b.P)}) == b.P
    assert same_bytes(got, b.singles(verifier))


def test_64_pairs(sift, verifier):
    seeds = U + T
    items = [(pc.scene(seeds[p % len(seeds)], 4 + p, p % 9, p % 3 == 0), (3 + p) if p % 5 == 0 else None, None)
             for p in range(64)]
    b = Batch(sift, items)
    assert b.rows <= 64 * 72
    got = b.run(verifier)
    b.check(got)
    assert same_bytes(got, b.singles(verifier))


def test_batch_two_runs_strides_and_another_stream(sift, verifier):
    import torch

    b = mixed(sift)
    a = b.run(verifier)
    assert same_bytes(a, b.run(verifier))
    assert same_bytes(a, mixed(sift, (5, 3)).run(verifier))
    assert same_bytes(a, b.run(verifier, stream=torch.cuda.Stream()))


def test_host_forms_and_module_functions(sift):
    key = (U[1], 300, 60, True)
    s, ref = pc.scene(*key), pc.reference(*key)
    m = s["matches"]
    v = sift.Verifier(len(m), 1)
    dm, dq, dt = dev(sift, m), dev(sift, s["q_xy"]), dev(sift, s["t_xy"])
    rec = record(sift, s["result"])[0]
    got, mask, points, recs, cands = v.recover_pose_homography_host(dm.value, 0, len(m), dq.value, len(s["q_xy"]), dt.value,
                                                                    len(s["t_xy"]), rec, s["mask"], s["cam_q"], s["cam_t"],
                                                                    q_stride=2, t_stride=2)
    assert got.tobytes() == pc.plane_pose_bytes(ref) and mask.tobytes() == ref["mask"].tobytes()
    assert points.view(np.uint32).tobytes() == ref["points"].view(np.uint32).tobytes()
    assert recs.tobytes() == ref["list"].tobytes() and cands.tobytes() == ref["candidates"].tobytes()
    R, t, mask2, points2, pose2, cands2 = sift.recoverPoseHomography(m, dq.value, dt.value, len(s["q_xy"]), len(s["t_xy"]),
                                                                     rec, s["mask"], s["cam_q"], s["cam_t"], des_stride=2,
                                                                     src_stride=2)
    assert R.shape == (3, 3) and R.tobytes() == ref["R"].tobytes() and t.tobytes() == ref["t"].tobytes()
    assert mask2.tobytes() == mask.tobytes() and points2.tobytes() == points.tobytes() and pose2.tobytes() == got.tobytes()
    assert cands2.tobytes() == cands.tobytes()
    R3, _, _, _, pose3, _ = sift.recoverPoseHomography(m, dq.value, dt.value, len(s["q_xy"]), len(s["t_xy"]),
                                                       s["H"].reshape(3, 3), None, s["cam_q"], s["cam_t"], des_stride=2,
                                                       src_stride=2)  # H alone, every match
    every = rule(s, mask=np.ones(len(m), np.uint8))
    assert pose3.tobytes() == pc.plane_pose_bytes(every) and R3.tobytes() == every["R"].tobytes()
    # the batched host form and module function
    b = mixed(sift)
    vb = sift.Verifier(b.rows, 1, b.P)
    dev_got = b.run(vb)
    verified = [(record(sift, r)[0], b.mask0[b.row0[p]: b.row0[p + 1]]) for p, r in enumerate(b.results)]
    host = vb.recover_pose_homography_batched_host(b.dm.value, b.dc.value, b.pairs, verified, b.cams_q, b.cams_t, q_stride=2,
                                                   t_stride=2)
    for p in range(b.P):
        a, n, k = int(b.row0[p]), b.n[p], int(dev_got["out_count"][p])
        rec_p, mask_p, points_p, recs_p, cands_p = host[p]
        assert rec_p.tobytes() == dev_got["pose"][p].tobytes(), p
        assert cands_p.tobytes() == dev_got["candidates"][p].tobytes(), p
        assert mask_p.tobytes() == dev_got["mask_out"][a:a + b.caps[p]].tobytes(), p
        assert points_p[:n].view(np.uint32).tobytes() == dev_got["points"][a:a + n].tobytes(), p
        assert recs_p.tobytes() == dev_got["out"][a:a + k].tobytes(), p
    full = [i for i, s in enumerate(b.scenes) if s is not None and b.n[i] == b.caps[i]]
    once = sift.recoverPoseHomographyBatched([b.scenes[i]["matches"] for i in full],
                                             [(b.scenes[i]["q_xy"], b.scenes[i]["t_xy"]) for i in full],
                                             [verified[i][0] for i in full], [verified[i][1] for i in full], b.cams_q[full],
                                             b.cams_t[full])
    for j, i in enumerate(full):
        assert once[j][4].tobytes() == dev_got["pose"][i].tobytes(), i
        assert once[j][2].tobytes() == dev_got["mask_out"][b.row0[i]: b.row0[i + 1]].tobytes(), i
        assert once[j][5].tobytes() == dev_got["candidates"][i].tobytes(), i


def test_refusals_launch_nothing(sift):
    b = mixed(sift)
    v = sift.Verifier(b.rows, 1, b.P)
    o = b.outputs()
    before = b.read(o)
    q, nq, t, nt, cap = b.pairs[1]
    a = int(b.row0[1])
    good = np.float32([500, 500, 320, 240])

    def one(cam_q=good, cam_t=good, **kw):
        v.recover_pose_homography_device(b.dm.value + 16 * a, 0, kw.get("cap", cap), q, nq, t, nt, kw.get("res", b.dres.value),
                                         kw.get("mask", b.dmask.value + a), cam_q, cam_t, kw.get("pose", o["pose"].value),
                                         o["mask_out"].value, o["points"].value, kw.get("out", o["out"].value), 0,
                                         o["candidates"].value, kw.get("max_depth", 50.0), kw.get("max_cos", 0.99998), 2, 2)

    inf, nan = float("inf"), float("nan")
    for kw, msg in ((dict(cam_q=np.float32([0, 500, 1, 1])), "fx and fy"), (dict(cam_t=np.float32([500, -1, 1, 1])), "fx and fy"),
                    (dict(cam_q=np.float32([inf, 500, 1, 1])), "fx and fy"), (dict(cam_t=np.float32([500, nan, 1, 1])), "fx and fy"),
                    (dict(cam_q=np.float32([500, 500, nan, 1])), "cx and cy"), (dict(cam_t=np.float32([500, 500, 1, inf])), "cx and cy"),
                    (dict(res=0), "result"), (dict(pose=0), "result"), (dict(max_depth=0.0), "max_depth"),
                    (dict(max_depth=-1.0), "max_depth"), (dict(max_depth=nan), "max_depth"), (dict(max_cos=1.5), "max_cos_parallax"),
                    (dict(max_cos=nan), "max_cos_parallax"), (dict(mask=0), "mask"), (dict(out=b.dm.value + 16 * a), "alias"),
                    (dict(cap=b.rows + 1), "max_matches")):
        with pytest.raises(sift.SiftHipError, match=msg):
            one(**kw)

    def many(pairs, cams_q=b.cams_q, **kw):
        v.recover_pose_homography_batched_device(b.dm.value, 0, pairs, b.dres.value, kw.get("mask", b.dmask.value), cams_q,
                                                 np.concatenate([b.cams_t, b.cams_t])[:len(pairs)], o["pose"].value,
                                                 o["mask_out"].value, o["points"].value, o["out"].value, 0,
                                                 o["candidates"].value, q_stride=2, t_stride=2)

    bad = b.cams_q.copy()
    bad[3, 1] = 0
    for pairs, kw, msg in ((b.pairs, dict(cams_q=bad), r"fx and fy.*pair 3"), (b.pairs, dict(mask=0), "mask"),
                           (b.pairs + [b.pairs[1]], dict(cams_q=np.concatenate([b.cams_q, b.cams_q[:1]])), "max_pairs"),
                           ([b.pairs[4]] * b.P, {}, "max_matches")):
        with pytest.raises(sift.SiftHipError, match=msg):
            many(pairs, **kw)
    sync(sift)
    assert same_bytes(before, b.read(o))


def test_pose_calls_leave_the_hypothesis_scratch_alone(sift):
    """What homography_hypotheses() answers after a verify call stays through plane pose calls."""
    s = pc.scene(U[5], 300, 60, True)
    n, K = len(s["matches"]), 64
    v = sift.Verifier(n, K)
    dm, dq, dt = dev(sift, s["matches"]), dev(sift, s["q_xy"]), dev(sift, s["t_xy"])
    res, mask = dev(sift, np.zeros(52, np.uint8)), dev(sift, np.zeros(n, np.uint8))
    v.verify_homography_device(dm.value, 0, n, dq.value, n, dt.value, n, res.value, 0, 0, mask.value, ec.MAX_ERROR, K, 0, 2, 2)
    before = v.homography_hypotheses()
    out = dev(sift, np.zeros(96, np.uint8))
    v.recover_pose_homography_device(dm.value, 0, n, dq.value, n, dt.value, n, res.value, mask.value, s["cam_q"], s["cam_t"],
                                     out.value, q_stride=2, t_stride=2)
    rec = res.to_numpy(sift.HOMOGRAPHY_RESULT_DTYPE, (1,))[0]
    v.recover_pose_homography_host(dm.value, 0, n, dq.value, n, dt.value, n, rec, mask.to_numpy(np.uint8, (n,)), s["cam_q"],
                                   s["cam_t"], q_stride=2, t_stride=2)
    after = v.homography_hypotheses()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and before[3].max() >= 300
    assert out.to_numpy(sift.PLANE_POSE_RESULT_DTYPE, (1,))[0]["candidate"] >= 0


CHAIN_K = 256


def run_chain(sift, v, d, st):
    """verify_homography_device -> refine_homography_device -> recover_pose_homography_device on stream st, no read in
    between."""
    s = d["s"]
    n = len(s["matches"])
    v.verify_homography_device(d["lst"].value, 0, n, d["qxy"].value, n, d["txy"].value, n, d["res"].value, 0, 0, d["mask"].value,
                               ec.MAX_ERROR, CHAIN_K, 3, 2, 2, stream=st)
    v.refine_homography_device(d["lst"].value, 0, n, d["qxy"].value, n, d["txy"].value, n, d["res"].value, d["mask"].value, 0, 0,
                               0, ec.MAX_ERROR, 2, 2, 2, stream=st)
    v.recover_pose_homography_device(d["lst"].value, 0, n, d["qxy"].value, n, d["txy"].value, n, d["res"].value, d["mask"].value,
                                     s["cam_q"], s["cam_t"], d["pose"].value, d["front"].value, d["points"].value,
                                     d["out"].value, d["out_count"].value, d["cands"].value, q_stride=2, t_stride=2, stream=st)


def chain_sizes(d):
    n = len(d["s"]["matches"])
    return dict(res=52, mask=n, pose=96, front=n, points=12 * n, out=16 * n, out_count=4, cands=256)


def chain_buffers(sift, max_pairs):
    s = pc.scene(U[0], 300, 60)
    n = len(s["matches"])
    v = sift.Verifier(n if max_pairs == 1 else 4 * n, CHAIN_K, max_pairs)
    d = dict(s=s, lst=dev(sift, s["matches"]), qxy=dev(sift, s["q_xy"]), txy=dev(sift, s["t_xy"]))
    for name, size in chain_sizes(d).items():
        d[name] = dev(sift, np.full(size, FILL, np.uint8))
    return v, d


def chain_outputs(sift, d):
    return {k: d[k].to_numpy(np.uint8, (size,)) for k, size in chain_sizes(d).items()}


def check_chain(sift, d, got):
    from sift_amd import cv

    s = d["s"]
    lst, k = s["matches"], len(s["matches"])
    ver = cv.ransac_homography(lst, s["q_xy"], s["t_xy"], ec.MAX_ERROR, CHAIN_K, 3)
    ref = cv.refine_homography(lst, s["q_xy"], s["t_xy"], ver, ec.MAX_ERROR, 2)
    want = cv.recover_pose_homography(lst, s["q_xy"], s["t_xy"], ref, ref["mask"], s["cam_q"], s["cam_t"])
    assert got["res"][:36].tobytes() == ref["H"].tobytes() and got["mask"].tobytes() == ref["mask"].tobytes()
    assert ref["inliers"] >= s["planted"]
    assert got["pose"].tobytes() == pc.plane_pose_bytes(want) and want["candidate"] >= 0 and want["in_front"] >= s["planted"]
    assert got["cands"].tobytes() == want["candidates"].tobytes()
    assert got["front"][:k].tobytes() == want["mask"].tobytes()
    assert got["points"][:12 * k].tobytes() == want["points"].tobytes()
    assert got["out_count"].view(np.int32)[0] == want["in_front"]
    assert got["out"][:16 * want["in_front"]].tobytes() == want["list"].tobytes()
    # the scene's pose, through a RANSAC H of noise-free points refitted on its inliers: far inside a milliradian
    e = pc.errors((want["R"], want["t"], want["normal"], want["distance"]), s["R"], s["t"], s["n"], s["d"])
    print("chain to truth", e)
    assert max(e) < 1e-3


def test_chain_on_one_stream_with_one_final_read(sift):
    import torch

    v, d = chain_buffers(sift, 1)
    stream = torch.cuda.Stream()
    run_chain(sift, v, d, stream.cuda_stream)
    stream.synchronize()
    check_chain(sift, d, chain_outputs(sift, d))


def test_chain_captured_in_a_graph_and_replayed(sift):
    """The same chain captured once, on a verifier made for batches (max_pairs > 1), and replayed twice: equal bytes,
    equal to the rule.  The device forms allocate nothing and synchronise nothing, so they capture as they are."""
    import torch

    v, d = chain_buffers(sift, 4)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        run_chain(sift, v, d, torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        for name, size in chain_sizes(d).items():  # every buffer the graph writes starts as FILL again
            fill = np.full(size, FILL, np.uint8)
            sift._check(sift.lib().sift_hip_memcpy_h2d(d[name].value, fill.ctypes.data, fill.size), "memcpy")
        graph.replay()
        torch.cuda.synchronize()
        runs.append(chain_outputs(sift, d))
    assert same_bytes(runs[0], runs[1])
    check_chain(sift, d, runs[0])


def test_the_pose_from_F_is_unchanged_after_plane_pose_calls(sift):
    """recover_pose_device on an F scene of tests/pose_cases.py returns the mirror's bytes after homography pose calls
    on the same verifier: the two share the gather scratch and nothing else."""
    h = pc.scene(U[0], 300, 60, True)
    f, ref = fc.scene(1, 1, 300, 60, True), fc.reference(1, 1, 300, 60, True)
    v = sift.Verifier(360, 1)
    check(pose(sift, h, v=v), pc.reference(U[0], 300, 60, True), h["matches"], 360)
    dm, dq, dt = dev(sift, f["matches"]), dev(sift, f["q_xy"]), dev(sift, f["t_xy"])
    rec = np.zeros(1, sift.VERIFY_RESULT_DTYPE)
    rec["F"][0], rec["hypothesis"][0] = f["F"], 0
    res, mask = dev(sift, rec), dev(sift, f["mask"])
    out = dict(pose=dev(sift, np.full(80 + GUARD, FILL, np.uint8)), front=dev(sift, np.zeros(360, np.uint8)),
               points=dev(sift, np.zeros(12 * 360, np.uint8)))
    v.recover_pose_device(dm.value, 0, 360, dq.value, 360, dt.value, 360, res.value, mask.value, f["cam_q"], f["cam_t"],
                          out["pose"].value, out["front"].value, out["points"].value, q_stride=2, t_stride=2)
    sync(sift)
    got = out["pose"].to_numpy(np.uint8, (80 + GUARD,))
    assert got[:80].tobytes() == fc.pose_bytes(ref) and (got[80:] == FILL).all() and ref["candidate"] >= 0
    assert out["front"].to_numpy(np.uint8, (360,)).tobytes() == ref["mask"].tobytes()
    assert out["points"].to_numpy(np.uint32, (360, 3)).tobytes() == ref["points"].view(np.uint32).tobytes()
    check(pose(sift, h, v=v), pc.reference(U[0], 300, 60, True), h["matches"], 360)
