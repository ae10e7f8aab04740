"""Essential-matrix verification on the GPU (sift_hip_verify_essential_*; k_verify_hypotheses_e in csrc/essential.hip,
and the existing gather, score and select kernels over its 10 K model slots).

The bar: what every sample drew, all 10 K models and valid flags, the counts, the result record, the mask, the inlier
list and its count equal sift_amd.cv.ransac_essential (the rule of include/sift_hip.h in numpy) as raw bytes, for the
single, batched, host and captured forms.  The inputs are tests/essential_cases.py; tests/test_essential_cases.py
checks the mirror itself on the CPU.
"""
import functools

import numpy as np
import pytest

import essential_cases as ec
import guided_cases as gc
import pose_cases as pc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs start as this byte: what the device does not write stays visible
S = ec.GPU_SEED


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def sync(sift):
    sift._check(sift.lib().sift_hip_device_sync(), "sync")


@functools.lru_cache(maxsize=None)
def mirror(planted, unrelated, K, seed=0, count=None, kind="general"):
    """cv.ransac_essential on the first `count` records (None: all) of a scene; read-only."""
    from sift_amd import cv

    s = ec.get(kind, S, planted, unrelated)
    m = s["matches"] if count is None else s["matches"][:max(count, 0)]
    return pc._freeze(cv.ransac_essential(m, s["q_xy"], s["t_xy"], s["cam_q"], s["cam_t"], ec.MAX_ERROR, K, seed))


class Job:
    """A scene's list and positions on the device, with prefilled outputs: verify_essential_device on them, and
    everything it wrote on the host."""

    def __init__(self, sift, s, K, count=None, cap=None, stride=(2, 2), v=None):
        self.sift, self.s, self.K, self.stride = sift, s, K, stride
        m = s["matches"]
        self.cap = cap = len(m) if cap is None else cap
        buf = np.zeros(cap, sift.DMATCH_DTYPE)
        buf[:len(m)] = m
        buf[len(m):]["queryIdx"] = -7  # records behind the list are never read
        self.buf = buf
        self.v = v or sift.Verifier(max(cap, 1), 1, essential_samples=K)
        self.dm = dev(sift, buf) if cap else None
        self.dq = dev(sift, gc.with_stride(s["q_xy"], stride[0])) if len(s["q_xy"]) else None
        self.dt = dev(sift, gc.with_stride(s["t_xy"], stride[1])) if len(s["t_xy"]) else None
        self.dc = dev(sift, np.int32([count])) if count is not None else None
        self.fresh()

    def fresh(self):
        s, cap = self.sift, max(self.cap, 1)
        self.res, self.mask = dev(s, np.full(52, FILL, np.uint8)), dev(s, np.full(cap, FILL, np.uint8))
        self.out, self.cnt = dev(s, np.full(16 * cap, FILL, np.uint8)), dev(s, np.full(4, FILL, np.uint8))

    def list_args(self):
        s = self.s
        return (self.dm.value if self.dm else 0, self.dc.value if self.dc else 0, self.cap,
                self.dq.value if self.dq else 0, len(s["q_xy"]), self.dt.value if self.dt else 0, len(s["t_xy"]))

    def read(self):
        s, cap = self.sift, max(self.cap, 1)
        return dict(result=self.res.to_numpy(s.VERIFY_RESULT_DTYPE, (1,))[0], out=self.out.to_numpy(s.DMATCH_DTYPE, (cap,)),
                    out_count=int(self.cnt.to_numpy(np.int32, (1,))[0]), mask=self.mask.to_numpy(np.uint8, (cap,)))

    def verify(self, seed=0, stream=None, getter=True):
        self.v.verify_essential_device(*self.list_args(), self.s["cam_q"], self.s["cam_t"], self.res.value, self.out.value,
                                       self.cnt.value, self.mask.value, ec.MAX_ERROR, self.K, seed, *self.stride,
                                       stream=stream)
        if not getter:
            return None
        samples, F, valid, counts = self.v.essential_hypotheses()  # synchronises
        return dict(self.read(), samples=samples, Fs=F, valid=valid, counts=counts)


def check_record(got, ref, buf):
    n, r = ref["matches"], got["result"]
    assert r["F"].tobytes() == ref["F"].tobytes(), (r["F"], ref["F"])
    assert (r["inliers"], r["hypothesis"], r["matches"], r["valid_hypotheses"]) == \
        (ref["inliers"], ref["hypothesis"], n, ref["valid_hypotheses"])
    assert got["out_count"] == ref["inliers"]
    assert got["out"][:ref["inliers"]].tobytes() == ref["list"].tobytes()
    assert got["out"][:ref["inliers"]].tobytes() == buf[:n][ref["mask"] != 0].tobytes()  # input records, input order
    assert (got["out"][ref["inliers"]:].view(np.uint8) == FILL).all()  # nothing behind the list is written
    assert np.array_equal(got["mask"][:n], ref["mask"])
    assert not got["mask"][n:len(buf)].any()  # every cap byte is written, zero behind the list


def check_against(got, ref, buf):
    """Every output of a verify call against cv.ransac_essential of the records that count."""
    assert got["samples"].shape == ref["samples"].shape and np.array_equal(got["samples"], ref["samples"])
    assert got["valid"].shape == ref["valid"].shape
    assert np.array_equal(got["valid"], ref["valid"]), np.flatnonzero(got["valid"] != ref["valid"])[:8]
    bad = np.flatnonzero((got["Fs"].view(np.uint32) != ref["Fs"].view(np.uint32)).any(1))
    assert got["Fs"].shape == ref["Fs"].shape and len(bad) == 0, (bad[:8], got["Fs"][bad[:1]], ref["Fs"][bad[:1]])
    assert np.array_equal(got["counts"], ref["counts"]), np.flatnonzero(got["counts"] != ref["counts"])[:8]
    check_record(got, ref, buf)


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "%d+%d" % s)
def test_shapes(sift, shape):
    s, ref = ec.scene(S, *shape), mirror(*shape, ec.K)
    job = Job(sift, s, ec.K)
    got = job.verify()
    print(shape, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid slots", ref["valid_hypotheses"])
    check_against(got, ref, job.buf)
    if sum(shape) < 5:
        assert got["result"]["hypothesis"] == -1 and got["out_count"] == 0 and not got["result"]["F"].any()
        assert (got["samples"] == -1).all() and not got["valid"].any() and not got["Fs"].any()
    else:
        assert ref["hypothesis"] >= 0 and ref["mask"][:shape[0]].all()
    if shape == ec.SHAPES[-1]:
        assert ref["inliers"] > 1024  # the list itself spans chunks of the compaction


@pytest.mark.parametrize("K", ec.GPU_KS)
def test_sample_counts_around_the_workgroup(sift, K):
    s, ref = ec.scene(S), mirror(ec.PLANTED, ec.UNRELATED, K)
    job = Job(sift, s, K)
    check_against(job.verify(), ref, job.buf)
    assert ref["Fs"].shape == (10 * K, 9) and ref["valid"].any()


@pytest.mark.parametrize("strides", [(2, 2), (3, 3)])
def test_strides_and_a_count_on_the_device(sift, strides):
    """The list at the head of a larger buffer, its length in a device counter (cap > count), under both strides."""
    s = ec.scene(S, 64, 1)
    job = Job(sift, s, 64, count=65, cap=97, stride=strides)
    check_against(job.verify(), mirror(64, 1, 64), job.buf)
    # a counter below the list's length clamps it, one above the cap is clamped to the cap; below 5: the empty result
    for count in (40, 10 ** 6, 5, 4, 0, -3):
        s2 = ec.scene(S)
        job = Job(sift, s2, 64, count=count, stride=strides)
        n = min(max(count, 0), 360)
        ref = mirror(ec.PLANTED, ec.UNRELATED, 64, 0, n)
        got = job.verify()
        check_against(got, ref, job.buf)
        if n < 5:
            r = got["result"]
            assert (r["hypothesis"], r["inliers"], r["matches"], r["valid_hypotheses"]) == (-1, 0, n, 0)


def test_two_runs_give_identical_bytes_seeds_differ_and_the_host_form_agrees(sift):
    s = ec.scene(S)
    job = Job(sift, s, ec.K)
    a = job.verify()
    job.fresh()
    b = job.verify()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes() if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    job.fresh()
    c = job.verify(seed=1)
    assert not np.array_equal(c["samples"], a["samples"]) and c["Fs"].tobytes() != a["Fs"].tobytes()
    check_against(c, mirror(ec.PLANTED, ec.UNRELATED, ec.K, 1), job.buf)
    # the host form, on the same verifier
    ref = mirror(ec.PLANTED, ec.UNRELATED, ec.K)
    F, inl, hyp = job.v.verify_essential_host(*job.list_args(), s["cam_q"], s["cam_t"], ec.MAX_ERROR, ec.K, 0, 2, 2)
    assert F.dtype == np.float32 and F.tobytes() == ref["F"].tobytes() == a["result"]["F"].tobytes()
    assert hyp == ref["hypothesis"] and inl.tobytes() == ref["list"].tobytes()
    rec, inl2, mask = job.v.verify_essential_host(*job.list_args(), s["cam_q"], s["cam_t"], ec.MAX_ERROR, ec.K, 0, 2, 2,
                                                  True)
    assert rec.tobytes() == a["result"].tobytes() and np.array_equal(mask, ref["mask"]) and inl2.tobytes() == inl.tobytes()
    # the one-shot function uploads the list itself and adds E
    from sift_amd import cv

    F2, inl3, hyp2, E = sift.verifyEssential(s["matches"], job.dq.value, job.dt.value, 360, 360, s["cam_q"], s["cam_t"],
                                             hypotheses=ec.K, des_stride=2, src_stride=2)
    assert F2.tobytes() == F.tobytes() and inl3.tobytes() == inl.tobytes() and hyp2 == hyp
    assert E.dtype == np.float64 and E.tobytes() == cv.essential_from_fundamental(F, s["cam_q"], s["cam_t"]).tobytes()
    F3, inl4, _, _ = sift.verifyEssential(s["matches"], job.dq.value, job.dt.value, 360, 360, s["cam_q"], s["cam_t"],
                                          hypotheses=ec.K, des_stride=2, src_stride=2, refit=1)
    fit = cv.refine_fundamental(s["matches"], s["q_xy"], s["t_xy"], ref, ec.MAX_ERROR, 1)
    assert F3.tobytes() == fit["F"].tobytes() and inl4.tobytes() == fit["list"].tobytes()


def test_bad_records_and_nan_positions(sift):
    from sift_amd import cv

    s = dict(ec.scene(S))
    m = s["matches"].copy()
    rows = np.arange(0, len(m), 7)
    m["queryIdx"][rows[0::3]] = -1
    m["queryIdx"][rows[1::3]] = 360
    m["trainIdx"][rows[2::3]] = 2 ** 30
    q = s["q_xy"].copy()
    q[m["queryIdx"][3], 0] = np.nan
    s["matches"], s["q_xy"] = m, q
    ref = cv.ransac_essential(m, q, s["t_xy"], s["cam_q"], s["cam_t"], ec.MAX_ERROR, ec.K, 0)
    job = Job(sift, s, ec.K)
    got = job.verify()
    check_against(got, ref, job.buf)
    assert not got["mask"][rows].any() and not got["mask"][3] and ref["hypothesis"] >= 0
    hit = np.isin(got["samples"], np.r_[rows, 3]).any(1)
    assert hit.any() and not got["valid"].reshape(-1, 10)[hit].any()  # a sample that holds one has no model


class Batch:
    """P pairs with ragged caps, their lists in one buffer with the counts on the device; pair `short` has fewer than
    5 matches.  Pair p: scene seed SEEDS[p % 4], its own cameras."""

    def __init__(self, sift, P, K, short=1):
        self.sift, self.P, self.K = sift, P, K
        sizes = [(300, 60), (3, 0), (63, 0), (64, 1), (120, 17), (5, 0), (40, 40)]
        self.scenes = [ec.scene(ec.SEEDS[p % 4], *sizes[p if P > 1 else 0]) for p in range(P)]
        self.n = [len(s["matches"]) for s in self.scenes]
        self.caps = [n + (5 * p) % 11 for p, n in enumerate(self.n)]  # ragged: cap >= n
        rows = sum(self.caps)
        buf = np.zeros(rows, sift.DMATCH_DTYPE)
        buf["queryIdx"] = -7
        self.row0 = np.concatenate([[0], np.cumsum(self.caps)]).astype(int)
        for p, s in enumerate(self.scenes):
            buf[self.row0[p]: self.row0[p] + self.n[p]] = s["matches"]
        self.buf = buf
        self.dm, self.dc = dev(sift, buf), dev(sift, np.int32(self.n))
        self.dq = [dev(sift, gc.with_stride(s["q_xy"], 2)) for s in self.scenes]
        self.dt = [dev(sift, gc.with_stride(s["t_xy"], 2)) for s in self.scenes]
        self.pairs = [(self.dq[p].value, len(s["q_xy"]), self.dt[p].value, len(s["t_xy"]), self.caps[p])
                      for p, s in enumerate(self.scenes)]
        self.cams_q = np.stack([s["cam_q"] for s in self.scenes])
        self.cams_t = np.stack([s["cam_t"] for s in self.scenes])
        self.v = sift.Verifier(rows, 1, max(P, 2), essential_samples=K)
        self.fresh()

    def fresh(self):
        s, rows = self.sift, len(self.buf)
        self.res, self.mask = dev(s, np.full(52 * self.P, FILL, np.uint8)), dev(s, np.full(rows, FILL, np.uint8))
        self.out, self.cnt = dev(s, np.full(16 * rows, FILL, np.uint8)), dev(s, np.full(4 * self.P, FILL, np.uint8))

    def run(self, seed=0, stream=None):
        self.v.verify_essential_batched_device(self.dm.value, self.dc.value, self.pairs, self.cams_q, self.cams_t,
                                               self.res.value, self.out.value, self.cnt.value, self.mask.value,
                                               ec.MAX_ERROR, self.K, seed, 2, 2, stream=stream)

    def read(self):
        s, rows = self.sift, len(self.buf)
        return dict(result=self.res.to_numpy(s.VERIFY_RESULT_DTYPE, (self.P,)), out=self.out.to_numpy(s.DMATCH_DTYPE, (rows,)),
                    out_count=self.cnt.to_numpy(np.int32, (self.P,)), mask=self.mask.to_numpy(np.uint8, (rows,)))

    def pair(self, got, p):
        a, b = self.row0[p], self.row0[p + 1]
        return dict(result=got["result"][p], out=got["out"][a:b], out_count=int(got["out_count"][p]), mask=got["mask"][a:b])

    def reference(self, p, seed=0):
        from sift_amd import cv

        s = self.scenes[p]
        return cv.ransac_essential(s["matches"], s["q_xy"], s["t_xy"], s["cam_q"], s["cam_t"], ec.MAX_ERROR, self.K, seed + p)


@pytest.mark.parametrize("P", (1, 3, 7))
def test_batched_pair_p_is_the_single_call_with_seed_plus_p(sift, P):
    K = 64
    b = Batch(sift, P, K)
    b.run(seed=5)
    sync(sift)
    got = b.read()
    for p in range(P):
        ref = b.reference(p, 5)
        check_record(b.pair(got, p), ref, b.buf[b.row0[p]: b.row0[p + 1]])
        if b.n[p] < 5:
            assert got["result"][p]["hypothesis"] == -1 and got["out_count"][p] == 0
    if P > 1:
        assert b.n[1] < 5 and got["result"][0]["hypothesis"] >= 0
    # the single call on pair 0's rows with the same seed: the same bytes
    s = b.scenes[0]
    job = Job(sift, s, K, count=b.n[0], cap=b.caps[0])
    one = job.verify(seed=5)
    pair0 = b.pair(got, 0)
    assert one["result"].tobytes() == pair0["result"].tobytes() and one["mask"].tobytes() == pair0["mask"].tobytes()
    assert one["out"].tobytes() == pair0["out"].tobytes() and one["out_count"] == pair0["out_count"]
    # the host form agrees
    host = b.v.verify_essential_batched_host(b.dm.value, b.dc.value, b.pairs, b.cams_q, b.cams_t, ec.MAX_ERROR, K, 5, 2, 2,
                                             True)
    for p, (rec, recs, mask) in enumerate(host):
        assert rec.tobytes() == got["result"][p].tobytes() and mask.tobytes() == b.pair(got, p)["mask"].tobytes()
        assert recs.tobytes() == b.pair(got, p)["out"][:rec["inliers"]].tobytes()


def test_a_pair_does_not_depend_on_its_neighbours(sift):
    K = 64
    b3, b7 = Batch(sift, 3, K), Batch(sift, 7, K)
    b3.run()
    b7.run()
    sync(sift)
    g3, g7 = b3.read(), b7.read()
    for p in range(3):  # the first three pairs are the same lists with the same caps and seeds
        a, c = b3.pair(g3, p), b7.pair(g7, p)
        assert a["result"].tobytes() == c["result"].tobytes() and a["mask"].tobytes() == c["mask"].tobytes()
        assert a["out"].tobytes() == c["out"].tobytes() and a["out_count"] == c["out_count"]
    # the getter belongs to single calls
    with pytest.raises(sift.SiftHipError, match="batch"):
        b3.v._e_hypotheses = K
        b3.v.essential_hypotheses()


CHAIN_K = 256


def chain_sizes(n):
    return dict(res=52, mask=n, out=16 * n, cnt=4, pose=80, front=n, points=12 * n)


def run_chain(job, d, st):
    """verify_essential_device -> recover_pose_device on stream st, no read in between."""
    s, n = job.s, job.cap
    job.v.verify_essential_device(*job.list_args(), s["cam_q"], s["cam_t"], d["res"].value, d["out"].value, d["cnt"].value,
                                  d["mask"].value, ec.MAX_ERROR, CHAIN_K, 2, 2, 2, stream=st)
    job.v.recover_pose_device(*job.list_args(), d["res"].value, d["mask"].value, s["cam_q"], s["cam_t"], d["pose"].value,
                              d["front"].value, d["points"].value, q_stride=2, t_stride=2, stream=st)


def check_chain(s, got):
    from sift_amd import cv

    m = s["matches"]
    ver = cv.ransac_essential(m, s["q_xy"], s["t_xy"], s["cam_q"], s["cam_t"], ec.MAX_ERROR, CHAIN_K, 2)
    want = cv.recover_pose(m, s["q_xy"], s["t_xy"], ver, ver["mask"], s["cam_q"], s["cam_t"])
    assert got["res"][:36].tobytes() == ver["F"].tobytes() and got["mask"].tobytes() == ver["mask"].tobytes()
    assert got["cnt"].view(np.int32)[0] == ver["inliers"] and got["out"][:16 * ver["inliers"]].tobytes() == ver["list"].tobytes()
    assert got["pose"].tobytes() == pc.pose_bytes(want) and want["candidate"] >= 0 and want["in_front"] >= s["planted"]
    assert got["front"].tobytes() == want["mask"].tobytes()
    assert got["points"].tobytes() == want["points"].view(np.uint8).tobytes()
    ra, ta = pc.rotation_angle(want["R"], s["R"]), pc.vector_angle(want["t"], s["t"])
    print("chain to truth: rotation %.3g translation %.3g" % (ra, ta))
    assert max(ra, ta) <= ec.POSE_TOL


def chain_job(sift, max_pairs=1):
    s = ec.scene(S)
    n = len(s["matches"])
    v = sift.Verifier(n if max_pairs == 1 else 4 * n, 1, max_pairs, essential_samples=CHAIN_K)
    job = Job(sift, s, CHAIN_K, v=v)
    return job, {k: dev(sift, np.full(size, FILL, np.uint8)) for k, size in chain_sizes(n).items()}


def test_chain_on_one_stream_with_one_final_read(sift):
    import torch

    job, d = chain_job(sift)
    stream = torch.cuda.Stream()
    run_chain(job, d, stream.cuda_stream)
    stream.synchronize()
    check_chain(job.s, {k: d[k].to_numpy(np.uint8, (size,)) for k, size in chain_sizes(job.cap).items()})


def test_chain_captured_in_a_graph_and_replayed(sift):
    """The chain captured once, on a verifier made for batches, and replayed twice: equal bytes, equal to the rule.
    After the reservation an essential call allocates nothing and synchronises nothing, so it captures as it is."""
    import torch

    job, d = chain_job(sift, 4)
    sizes = chain_sizes(job.cap)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        run_chain(job, d, torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        for name, size in sizes.items():  # every buffer the graph writes starts as FILL again
            fill = np.full(size, FILL, np.uint8)
            sift._check(sift.lib().sift_hip_memcpy_h2d(d[name].value, fill.ctypes.data, fill.size), "memcpy")
        graph.replay()
        torch.cuda.synchronize()
        runs.append({k: d[k].to_numpy(np.uint8, (size,)) for k, size in sizes.items()})
    assert all(runs[0][k].tobytes() == runs[1][k].tobytes() for k in sizes)
    check_chain(job.s, runs[0])


def test_scratch_boundary_and_the_reservation(sift):
    """A verifier reserved for S samples serves K = S and refuses K = S + 1, and one that has not reserved refuses every
    essential call, with the state error and nothing written; the fundamental calls on the same verifier are untouched."""
    from sift_amd import cv

    s = ec.scene(S)
    Sm = 65
    job = Job(sift, s, Sm)
    check_against(job.verify(), mirror(ec.PLANTED, ec.UNRELATED, Sm), job.buf)
    job.fresh()
    job.K = Sm + 1
    with pytest.raises(sift.SiftHipError, match="reservation") as e:
        job.verify()
    assert "(-3)" in str(e.value)  # SIFT_HIP_ERR_STATE
    sync(sift)
    got = job.read()
    assert (got["result"].tobytes() == bytes([FILL]) * 52) and (got["mask"] == FILL).all()
    assert (got["out"].view(np.uint8) == FILL).all() and got["out_count"] == int.from_bytes(bytes([FILL]) * 4, "little")
    with pytest.raises(sift.SiftHipError, match="essential scratch"):
        job.v.reserve_essential(8)  # once
    bare = Job(sift, s, 8, v=sift.Verifier(360, 8))
    with pytest.raises(sift.SiftHipError, match="no essential scratch"):
        bare.verify()
    sync(sift)
    assert bare.read()["result"].tobytes() == bytes([FILL]) * 52
    # a verifier with max_hypotheses = 1 serves essential calls of its reservation, and its fundamental call is the
    # mirror's after them
    v = job.v
    res, mask = dev(sift, np.full(52, FILL, np.uint8)), dev(sift, np.full(360, FILL, np.uint8))
    v.verify_device(*job.list_args(), res.value, 0, 0, mask.value, ec.MAX_ERROR, 1, 0, 2, 2)
    sync(sift)
    ref = cv.ransac_fundamental(s["matches"], s["q_xy"], s["t_xy"], ec.MAX_ERROR, 1, 0)
    assert res.to_numpy(np.uint8, (36,)).tobytes() == ref["F"].tobytes()
    assert mask.to_numpy(np.uint8, (360,)).tobytes() == ref["mask"].tobytes()
    with pytest.raises(sift.SiftHipError):
        v.essential_hypotheses()  # the last verify call was a fundamental call


WIDE = (75, 225, 1024)  # the budget list at K = 1024: 10,240 slots, past the 4096 a 12-bit index holds


@pytest.mark.parametrize("seed", (3, 6))
def test_slots_past_4096_and_a_winner_among_them(sift, seed):
    """The select's 64-bit key: on 75 planted + 225 unrelated records clean samples are rare, and under these seeds the
    winner sits in slot 7341 and 9134."""
    planted, unrelated, K = WIDE
    s, ref = ec.scene(S, planted, unrelated), mirror(planted, unrelated, K, seed)
    assert ref["hypothesis"] >= 4096 and ref["valid_hypotheses"] > 4096
    assert (ref["counts"][:4096] < ref["inliers"]).all()  # no slot a 12-bit index could name counts as many
    job = Job(sift, s, K)
    got = job.verify(seed=seed)
    print("seed", seed, "winner", ref["hypothesis"], "inliers", ref["inliers"], "valid slots", ref["valid_hypotheses"])
    check_against(got, ref, job.buf)


def test_the_other_getters_refuse_after_an_essential_call(sift):
    """After verify_essential_device the fundamental, homography and affine getters each return the state error and
    write nothing; after a call of their own model they answer again and the essential getter refuses."""
    s = ec.scene(S)
    K = 16
    job = Job(sift, s, K, v=sift.Verifier(360, K, essential_samples=K))
    job.verify()
    v, L = job.v, sift.lib()
    smp, mod, cnt = np.full((K, 8), FILL, np.int32), np.full((K, 9), FILL, np.float32), np.full(K, FILL, np.int32)
    ptrs = (smp.ctypes.data, mod.ctypes.data, cnt.ctypes.data)
    for rc in (L.sift_hip_verify_hypotheses_host(v._v, *ptrs, K), L.sift_hip_verify_homography_hypotheses_host(v._v, *ptrs, K),
               L.sift_hip_verify_affine_hypotheses_host(v._v, sift.MODEL_AFFINE, *ptrs, K),
               L.sift_hip_verify_affine_hypotheses_host(v._v, sift.MODEL_SIMILARITY, *ptrs, K)):
        assert rc == -3 and b"other model" in L.sift_hip_last_error()  # SIFT_HIP_ERR_STATE
    assert (smp == FILL).all() and (mod == FILL).all() and (cnt == FILL).all()  # nothing was written
    v._hypotheses = v._h_hypotheses = v._a_hypotheses = K
    for getter in (v.hypotheses, v.homography_hypotheses, v.affine_hypotheses, lambda: v.affine_hypotheses(True)):
        with pytest.raises(sift.SiftHipError, match="other model"):
            getter()
    res = dev(sift, np.full(52, FILL, np.uint8))
    v.verify_homography_device(*job.list_args(), res.value, hypotheses=K, q_stride=2, t_stride=2)
    assert v.homography_hypotheses()[0].shape == (K, 4)
    with pytest.raises(sift.SiftHipError, match="other model"):
        v.essential_hypotheses()
    job.fresh()
    assert job.verify()["samples"].shape == (K, 5)  # and back


def test_one_shot_batched_pair_p_is_the_one_shot_with_seed_plus_p(sift):
    """sift_amd.verifyEssentialBatched against verifyEssential pair by pair, with and without a refit round."""
    K, seed = 64, 3
    scenes = [ec.scene(ec.SEEDS[0]), ec.scene(ec.SEEDS[1], 3, 0), ec.scene(ec.SEEDS[2], 63, 0)]
    lists = [s["matches"] for s in scenes]
    xy = [(s["q_xy"], s["t_xy"]) for s in scenes]
    cq, ct = [s["cam_q"] for s in scenes], [s["cam_t"] for s in scenes]
    for refit in (0, 1):
        got = sift.verifyEssentialBatched(lists, xy, cq, ct, ec.MAX_ERROR, K, seed, refit)
        assert len(got) == 3
        for p, (s, (F, recs, hyp, E)) in enumerate(zip(scenes, got)):
            dq, dt = dev(sift, s["q_xy"]), dev(sift, s["t_xy"])
            F1, recs1, hyp1, E1 = sift.verifyEssential(s["matches"], dq.value, dt.value, len(s["q_xy"]), len(s["t_xy"]),
                                                       s["cam_q"], s["cam_t"], ec.MAX_ERROR, K, seed + p, 2, 2, refit)
            assert F.tobytes() == F1.tobytes() and recs.tobytes() == recs1.tobytes() and hyp == hyp1, (refit, p)
            assert E.tobytes() == E1.tobytes()
        assert got[1][2] == -1 and not got[1][0].any() and got[0][2] >= 0 and got[2][2] >= 0
