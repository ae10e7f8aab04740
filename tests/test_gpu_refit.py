"""The refit of a verified model on the GPU (sift_hip_refine_*; kernels in csrc/refit.hip), both models.

The bar: the result record, the mask, the inlier records, their count and the number of accepted rounds equal
sift_amd.cv.refine_fundamental / refine_homography (the rule of include/sift_hip.h in numpy float64) as raw bytes, in
the single-pair and the batched form, and nothing else is written.  A call starts from the verified state of the numpy
rule, uploaded -- tests/test_gpu_verify*.py hold the verify calls to the same rule --, except in the chain test, where
the device's own verify call feeds it.  The inputs are tests/refit_cases.py; tests/test_refit_cases.py checks the mirror
itself on the CPU.
"""
import numpy as np
import pytest

import epipolar_cases as ec
import homography_cases as hc
import refit_cases as rc
import verify_batched_cases as bc

pytestmark = pytest.mark.gpu
FILL = 0x5A  # the outputs, and the bytes no call may touch, start as this byte
GUARD = 96


def dev(sift, a):
    return sift.DeviceArray.from_numpy(np.ascontiguousarray(a))


def dtype_of(sift, model):
    return sift.VERIFY_RESULT_DTYPE if model == "fundamental" else sift.HOMOGRAPHY_RESULT_DTYPE


def record(sift, model, d):
    """The 52-byte result record of a ransac / refine dict."""
    r = np.zeros(1, dtype_of(sift, model))
    r[rc.FIELD[model]][0] = d[rc.FIELD[model]]
    for k in ("inliers", "hypothesis", "matches", "valid_hypotheses"):
        r[k][0] = d[k]
    return r


def single(v, model):
    return v.refine_device if model == "fundamental" else v.refine_homography_device


def batched(v, model):
    return v.refine_batched_device if model == "fundamental" else v.refine_homography_batched_device


def refine(sift, model, buf, q_xy, t_xy, state, rounds, count=None, stride=(2, 2), v=None, max_error=rc.MAX_ERROR):
    """refine_device on an uploaded list and verified state; everything it may write, back on the host.  The mask bytes
    and out rows past the n records that count start as FILL."""
    cap = len(buf)
    n = cap if count is None else count
    v = v or sift.Verifier(max(cap, 1), 16)
    dm = dev(sift, buf) if cap else None
    dq, dt = dev(sift, ec.with_stride(q_xy, stride[0])), dev(sift, ec.with_stride(t_xy, stride[1]))
    dc = dev(sift, np.int32([count])) if count is not None else None
    mask0 = np.full(cap + GUARD, FILL, np.uint8)
    mask0[:n] = state["mask"]
    res, mask = dev(sift, record(sift, model, state)), dev(sift, mask0)
    out = dev(sift, np.full(16 * (cap + GUARD), FILL, np.uint8))
    cnt, acc = dev(sift, np.full(4, FILL, np.uint8)), dev(sift, np.full(4, FILL, np.uint8))
    single(v, model)(dm.value if dm else 0, dc.value if dc else 0, cap, dq.value, len(q_xy), dt.value, len(t_xy), res.value,
                     mask.value, out.value, cnt.value, acc.value, max_error, rounds, stride[0], stride[1])
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    return dict(result=res.to_numpy(dtype_of(sift, model), (1,)), mask=mask.to_numpy(np.uint8, (cap + GUARD,)),
                out=out.to_numpy(sift.DMATCH_DTYPE, (cap + GUARD,)), out_count=int(cnt.to_numpy(np.int32, (1,))[0]),
                accepted=int(acc.to_numpy(np.int32, (1,))[0]))


def check(sift, model, got, ref, buf, n):
    """Every output of a refine call against the numpy rule's dict."""
    want = record(sift, model, ref)
    assert got["result"].tobytes() == want.tobytes(), (got["result"], want)
    assert got["accepted"] == ref["accepted"]
    assert np.array_equal(got["mask"][:n], ref["mask"])
    assert (got["mask"][n:] == FILL).all()  # bytes at and past n are not written
    k = int((ref["mask"] != 0).sum())
    assert got["out_count"] == k == len(ref["list"])
    assert got["out"][:k].tobytes() == ref["list"].tobytes() == buf[:n][ref["mask"] != 0].tobytes()
    assert (got["out"][k:].view(np.uint8) == FILL).all()


CASES = [(m, s, r) for m in rc.MODELS for s in rc.shapes(m) for r in rc.ROUNDS]


@pytest.mark.parametrize("model,shape,rounds", CASES, ids=["%s-%d+%d-r%d" % (m, s[0], s[1], r) for m, s, r in CASES])
def test_shapes(sift, model, shape, rounds):
    mod = rc.CASES[model]
    m, q_xy, t_xy, _ = mod.case(*shape[:2])
    ref = rc.refined(model, shape, rounds)
    if shape == mod.CAPPED:  # the list at the head of a larger buffer, its length on the device
        buf, count = mod.capped(), len(m)
    else:
        buf, count = m, None
    got = refine(sift, model, buf, q_xy, t_xy, rc.verified(model, shape), rounds, count=count)
    print(model, shape, "rounds", rounds, "inliers", rc.verified(model, shape)["inliers"], "->", ref["inliers"],
          "accepted", ref["accepted"])
    check(sift, model, got, ref, buf, len(m))
    if shape[0] + shape[1] < rc.NEED[model]:
        assert got["accepted"] == 0 and got["out_count"] == 0 and got["result"]["hypothesis"][0] == -1


@pytest.mark.parametrize("strides", [(3, 3), (5, 2)])
@pytest.mark.parametrize("model", rc.MODELS)
def test_strides_give_identical_results(sift, model, strides):
    for shape in (rc.CASES[model].MAIN, (24, 9, 256)):
        m, q_xy, t_xy, _ = rc.CASES[model].case(*shape[:2])
        got = refine(sift, model, m, q_xy, t_xy, rc.verified(model, shape), 3, stride=strides)
        check(sift, model, got, rc.refined(model, shape, 3), m, len(m))


@pytest.mark.parametrize("model", rc.MODELS)
def test_nan_position_fit_minimum_and_unusable_records(sift, model):
    refine_rule = rc.rules(model)[2]
    f = rc.FIELD[model]
    # a masked record whose position is NaN is skipped
    m, q_nan, t_xy, state, j = rc.nan_case(model)
    ref = refine_rule(m, q_nan, t_xy, state, rc.MAX_ERROR, 2)
    check(sift, model, refine(sift, model, m, q_nan, t_xy, state, 2), ref, m, len(m))
    # one fit record fewer than the minimum, and exactly the minimum
    mod = rc.CASES[model]
    m, q_xy, t_xy, _ = mod.case(*mod.MAIN[:2])
    r0 = rc.verified(model, mod.MAIN)
    inl = np.flatnonzero(r0["mask"])
    for keep in (rc.NEED[model] - 1, rc.NEED[model]):
        mask = np.zeros(len(m), np.uint8)
        mask[inl[:keep]] = 1
        state = dict(r0, mask=mask, inliers=keep)
        ref = refine_rule(m, q_xy, t_xy, state, rc.MAX_ERROR, 2)
        got = refine(sift, model, m, q_xy, t_xy, state, 2)
        check(sift, model, got, ref, m, len(m))
        if keep < rc.NEED[model]:
            assert got["accepted"] == 0 and got["result"].tobytes() == record(sift, model, state).tobytes()
    # an emptied record, a zero model and a model with a NaN stay, whatever the mask says
    for state in (dict(r0, hypothesis=-1), dict(r0, **{f: np.zeros(9, np.float32)}),
                  dict(r0, **{f: np.r_[r0[f][:8], np.float32(np.nan)].astype(np.float32)})):
        ref = refine_rule(m, q_xy, t_xy, state, rc.MAX_ERROR, 1)
        got = refine(sift, model, m, q_xy, t_xy, state, 1)
        check(sift, model, got, ref, m, len(m))
        assert got["accepted"] == 0 and got["result"].tobytes() == record(sift, model, state).tobytes()


class Batch:
    """A batch of tests/verify_batched_cases.py on the device with the verified state of every pair: the numpy rule's
    with the seed + p.  The mask bytes between a pair's n and its cap hold FILL."""

    def __init__(self, sift, model, name, pairs=None, stride=(2, 2)):
        self.sift, self.model, self.name, self.stride = sift, model, name, stride
        self.idx = list(range(len(bc.pairs(model, name)))) if pairs is None else list(pairs)
        self.host = [bc.pairs(model, name)[p] for p in self.idx]
        self.state = [bc.reference(model, name, p) for p in self.idx]
        self.caps = [len(p["buf"]) for p in self.host]
        self.row0 = np.concatenate([[0], np.cumsum(self.caps)]).astype(int)
        self.P, self.rows = len(self.host), int(self.row0[-1])
        self.dm = dev(sift, np.concatenate([p["buf"] for p in self.host]))
        self.dc = dev(sift, np.int32([p["count"] for p in self.host]))
        self.dxy = [(dev(sift, ec.with_stride(p["q_xy"], stride[0])), dev(sift, ec.with_stride(p["t_xy"], stride[1])))
                    if len(p["buf"]) else None for p in self.host]
        self.pairs = [(d[0].value, len(p["q_xy"]), d[1].value, len(p["t_xy"]), cap) if d else (0, 0, 0, 0, 0)
                      for p, d, cap in zip(self.host, self.dxy, self.caps)]
        self.mask0 = np.full(self.rows + GUARD, FILL, np.uint8)
        for p, s in enumerate(self.state):
            self.mask0[self.row0[p]: self.row0[p] + s["matches"]] = s["mask"]
        self.res0 = np.concatenate([record(sift, model, s) for s in self.state] +
                                   [np.frombuffer(bytes([FILL]) * 52, dtype_of(sift, model))])

    def outputs(self):
        s = self.sift
        return dict(res=dev(s, self.res0), mask=dev(s, self.mask0), out=dev(s, np.full(16 * (self.rows + GUARD), FILL, np.uint8)),
                    cnt=dev(s, np.full(4 * (self.P + 1), FILL, np.uint8)), acc=dev(s, np.full(4 * (self.P + 1), FILL, np.uint8)))

    def read(self, o):
        s = self.sift
        return dict(results=o["res"].to_numpy(dtype_of(s, self.model), (self.P + 1,)),
                    mask=o["mask"].to_numpy(np.uint8, (self.rows + GUARD,)),
                    out=o["out"].to_numpy(s.DMATCH_DTYPE, (self.rows + GUARD,)),
                    out_counts=o["cnt"].to_numpy(np.int32, (self.P + 1,)), accepted=o["acc"].to_numpy(np.int32, (self.P + 1,)))

    def run(self, v, rounds, stream=None):
        o = self.outputs()
        batched(v, self.model)(self.dm.value, self.dc.value, self.pairs, o["res"].value, o["mask"].value, o["out"].value,
                               o["cnt"].value, o["acc"].value, bc.MAX_ERROR, rounds, self.stride[0], self.stride[1],
                               stream.cuda_stream if stream else None)
        if stream:
            stream.synchronize()
        else:
            self.sift._check(self.sift.lib().sift_hip_device_sync(), "sync")
        return self.read(o)

    def singles(self, v, rounds):
        """The same pairs through P single-pair calls on the same verifier, laid out as the batch."""
        o = self.outputs()
        for p, (q, nq, t, nt, cap) in enumerate(self.pairs):
            a = int(self.row0[p])
            single(v, self.model)(self.dm.value + 16 * a if cap else 0, self.dc.value + 4 * p, cap, q, nq, t, nt,
                                  o["res"].value + 52 * p, o["mask"].value + a, o["out"].value + 16 * a,
                                  o["cnt"].value + 4 * p, o["acc"].value + 4 * p, bc.MAX_ERROR, rounds, self.stride[0],
                                  self.stride[1])
        self.sift._check(self.sift.lib().sift_hip_device_sync(), "sync")
        return self.read(o)

    def check(self, got, rounds):
        refine_rule = rc.rules(self.model)[2]
        for p, (pr, s) in enumerate(zip(self.host, self.state)):
            n, a, cap = s["matches"], int(self.row0[p]), self.caps[p]
            ref = refine_rule(pr["buf"][:n], pr["q_xy"], pr["t_xy"], s, bc.MAX_ERROR, rounds)
            assert got["results"][p:p + 1].tobytes() == record(self.sift, self.model, ref).tobytes(), p
            assert got["accepted"][p] == ref["accepted"], p
            mask, rows = got["mask"][a:a + cap], got["out"][a:a + cap]
            assert np.array_equal(mask[:n], ref["mask"]) and (mask[n:] == FILL).all(), p  # the gap keeps its canary
            k = len(ref["list"])
            assert got["out_counts"][p] == k and rows[:k].tobytes() == ref["list"].tobytes(), p
            assert (rows[k:].view(np.uint8) == FILL).all(), p
        for key in ("results", "out_counts", "accepted"):
            assert (got[key][self.P:].view(np.uint8) == FILL).all(), key
        assert (got["out"][self.rows:].view(np.uint8) == FILL).all() and (got["mask"][self.rows:] == FILL).all()


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture(scope="module")
def verifier(sift):
    rows = max(int(bc.row0(m, b)[-1]) for m in bc.MODELS for b in ("MIXED", "FULL"))
    return sift.Verifier(rows, 16, 64)


@pytest.mark.parametrize("rounds", rc.ROUNDS)
@pytest.mark.parametrize("batch,pairs", [("MIXED", None), ("MIXED", (0, 1, 2)), ("FULL", None)], ids=["P7", "P3", "P64"])
@pytest.mark.parametrize("model", rc.MODELS)
def test_every_pair_equals_the_rule_and_the_single_call(sift, verifier, model, batch, pairs, rounds):
    """MIXED holds a pair below the minimum, an empty pair, the capped buffer and the 2113-record list; its first three
    pairs are the P = 3 batch; FULL is the most a call takes."""
    b = Batch(sift, model, batch, pairs)
    got = b.run(verifier, rounds)
    b.check(got, rounds)
    assert same_bytes(got, b.singles(verifier, rounds))


@pytest.mark.parametrize("model", rc.MODELS)
def test_two_runs_strides_and_another_stream(sift, verifier, model):
    import torch

    b = Batch(sift, model, "MIXED")
    a = b.run(verifier, 2)
    assert same_bytes(a, b.run(verifier, 2))
    b.check(a, 2)
    wide = Batch(sift, model, "MIXED", stride=(3, 3))
    assert same_bytes(a, wide.run(verifier, 2))
    s = torch.cuda.Stream()
    assert same_bytes(a, b.run(verifier, 2, stream=s))


@pytest.mark.parametrize("model", rc.MODELS)
def test_host_forms_and_module_functions(sift, model):
    mod = rc.CASES[model]
    shape = mod.MAIN
    m, q_xy, t_xy, _ = mod.case(*shape[:2])
    f = rc.FIELD[model]
    ref = rc.refined(model, shape, 2)
    v = sift.Verifier(len(m), shape[2])
    dm, dq, dt = dev(sift, m), dev(sift, q_xy), dev(sift, t_xy)
    args = (dm.value, 0, len(m), dq.value, len(q_xy), dt.value, len(t_xy))
    verify = v.verify_host if model == "fundamental" else v.verify_homography_host
    host = v.refine_host if model == "fundamental" else v.refine_homography_host
    r, _, mask = verify(*args, rc.MAX_ERROR, shape[2], 0, 2, 2, True)
    r2, recs, mask2, accepted = host(*args, r, mask, rc.MAX_ERROR, 2, 2, 2)
    assert r2.tobytes() == record(sift, model, ref)[0].tobytes() and accepted == ref["accepted"]
    assert mask2.tobytes() == ref["mask"].tobytes() and recs.tobytes() == ref["list"].tobytes()
    fn = sift.verifyFundamental if model == "fundamental" else sift.verifyHomography
    M, recs3, hyp = fn(m, dq.value, dt.value, len(q_xy), len(t_xy), rc.MAX_ERROR, shape[2], 0, 2, 2, refit=2)
    assert M.shape == (3, 3) and M.tobytes() == ref[f].tobytes() and recs3.tobytes() == recs.tobytes()
    assert hyp == ref["hypothesis"]
    M0, _, _ = fn(m, dq.value, dt.value, len(q_xy), len(t_xy), rc.MAX_ERROR, shape[2], 0, 2, 2)  # refit = 0: as before
    assert M0.tobytes() == rc.verified(model, shape)[f].tobytes()
    # the batched host form and module function on the P = 3 batch
    b = Batch(sift, model, "MIXED", (0, 1, 2))
    vb = sift.Verifier(b.rows, 256, 3)
    K, seed = bc.BATCHES["MIXED"]
    vhost = vb.verify_batched_host if model == "fundamental" else vb.verify_homography_batched_host
    rhost = vb.refine_batched_host if model == "fundamental" else vb.refine_homography_batched_host
    verified = vhost(b.dm.value, b.dc.value, b.pairs, bc.MAX_ERROR, K, seed, 2, 2, True)
    refined = rhost(b.dm.value, b.dc.value, b.pairs, verified, bc.MAX_ERROR, 2, 2, 2)
    got = b.run(vb, 2)
    fnb = sift.verifyFundamentalBatched if model == "fundamental" else sift.verifyHomographyBatched
    once = fnb([p["buf"][:p["count"]] for p in b.host], [(p["q_xy"], p["t_xy"]) for p in b.host], bc.MAX_ERROR, K, seed,
               refit=2)
    for p in range(b.P):
        a, k = int(b.row0[p]), int(got["out_counts"][p])
        rec, recs, mask, acc = refined[p]
        assert rec.tobytes() == got["results"][p].tobytes() and acc == got["accepted"][p]
        assert recs.tobytes() == got["out"][a:a + k].tobytes()
        assert mask[:b.state[p]["matches"]].tobytes() == got["mask"][a:a + b.state[p]["matches"]].tobytes()
        assert once[p][0].tobytes() == rec[f].tobytes() and once[p][1].tobytes() == recs.tobytes()


def test_refusals_launch_nothing(sift):
    model = "fundamental"
    b = Batch(sift, model, "MIXED", (0, 1, 2))
    v = sift.Verifier(b.rows, 16, 3)
    o = b.outputs()
    before = b.read(o)
    q, nq, t, nt, cap = b.pairs[1]
    a = int(b.row0[1])
    one = lambda **kw: v.refine_device(b.dm.value + 16 * a, 0, kw.get("cap", cap), q, nq, t, nt,  # noqa: E731
                                       kw.get("res", o["res"].value), kw.get("mask", o["mask"].value),
                                       kw.get("out", o["out"].value), 0, 0, kw.get("e", 1.5), kw.get("rounds", 1), 2, 2)
    for kw, msg in ((dict(rounds=0), "rounds"), (dict(rounds=9), "rounds"), (dict(mask=0), "mask"), (dict(res=0), "result"),
                    (dict(e=0.0), "max_error"), (dict(out=b.dm.value + 16 * a), "alias"), (dict(cap=b.rows + 1), "max_matches")):
        with pytest.raises(sift.SiftHipError, match=msg):
            one(**kw)
    many = lambda pairs, **kw: v.refine_batched_device(b.dm.value, 0, pairs, o["res"].value, kw.get("mask", o["mask"].value),  # noqa: E731
                                                       o["out"].value, 0, 0, 1.5, kw.get("rounds", 1), 2, 2)
    for pairs, kw, msg in ((b.pairs, dict(rounds=9), "rounds"), (b.pairs, dict(mask=0), "mask"),
                           (b.pairs + [b.pairs[1]], {}, "max_pairs"), ([b.pairs[1]] * 3, {}, "max_matches")):
        with pytest.raises(sift.SiftHipError, match=msg):
            many(pairs, **kw)
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    assert same_bytes(before, b.read(o))


@pytest.mark.parametrize("model", ["homography", "fundamental"])
def test_chain_on_one_stream(sift, model):
    """match_list_batched -> verify_*_batched_device -> refine_*_batched_device -> the guided rematch reading the
    refined records at stride 52 (the homography through project_homography_batched_device), on one stream with no
    read-back until the end: the refined records and the rematch equal the numpy chain of each pair."""
    import torch

    import test_gpu_match_guided_batched as gb
    from sift_amd import cv

    K, seed, radius, rounds = 256, 5, 2.0, 2
    homography = model == "homography"
    make = gb.planted_pair if homography else (lambda nq, nt, s: gb.planted_pair(nq, nt, s, ec.project_pairs))
    pairs = gb.chain_pairs(make, gb.CHAIN_SHAPES)
    up = gb.Uploaded(sift, pairs, 3, 3)
    P, rows = len(pairs), up.rows
    m, v = sift.Matcher(400, 400, max_pairs=2 * P), sift.Verifier(rows, K, P)
    lst, cnt = gb.Guarded(sift, rows, sift.DMATCH_DTYPE), gb.Guarded(sift, P, np.int32)
    res, mask = gb.Guarded(sift, P, sift.VERIFY_RESULT_DTYPE), gb.Guarded(sift, (rows + 3) // 4, np.int32)
    acc = gb.Guarded(sift, P, np.int32)
    proj = [gb.Guarded(sift, n, np.float32, 2) for n in up.nq]
    out2, cnt2 = gb.Guarded(sift, rows, sift.DMATCH_DTYPE), gb.Guarded(sift, P, np.int32)
    warm, wcnt = dev(sift, np.zeros(16 * rows, np.uint8)), dev(sift, np.zeros(4 * P, np.uint8))
    m.match_list_batched(*up.sets(), warm.value, wcnt.value)  # the matcher's first list call allocates
    sift._check(sift.lib().sift_hip_device_sync(), "sync")
    vpairs = [(a, n, b, k, n) for a, n, b, k in up.positions()]
    s = torch.cuda.Stream()
    st = s.cuda_stream
    m.match_list_batched(*up.sets(), lst.value, cnt.value, stream=st)
    if homography:
        v.verify_homography_batched_device(lst.value, cnt.value, vpairs, res.value, 0, 0, mask.value, hc.MAX_ERROR, K, seed,
                                           3, 3, stream=st)
        v.refine_homography_batched_device(lst.value, cnt.value, vpairs, res.value, mask.value, 0, 0, acc.value,
                                           hc.MAX_ERROR, rounds, 3, 3, stream=st)
        sift.project_homography_batched_device(res.value, [(a.value, n, o.value) for a, n, o in zip(up.qxy, up.nq, proj)],
                                               3, 2, 52, stream=st)
        pos = [(o.value, n, b.value, k) for o, n, b, k in zip(proj, up.nq, up.txy, up.nt)]
        m.match_list_guided_batched(*up.sets(), pos, radius, out2.value, cnt2.value, 2, 3, stream=st)
    else:
        v.verify_batched_device(lst.value, cnt.value, vpairs, res.value, 0, 0, mask.value, ec.MAX_ERROR, K, seed, 3, 3,
                                stream=st)
        v.refine_batched_device(lst.value, cnt.value, vpairs, res.value, mask.value, 0, 0, acc.value, ec.MAX_ERROR, rounds,
                                3, 3, stream=st)
        m.match_list_epipolar_batched(*up.sets(), up.positions(), res.value, ec.MAX_ERROR, out2.value, cnt2.value, gb.INF,
                                      52, 3, 3, stream=st)
    s.synchronize()
    (r, ok1), (got_acc, ok2), (rec2, ok3), (n2, ok4), (mk, ok5) = res.read(), acc.read(), out2.read(), cnt2.read(), mask.read()
    assert ok1 and ok2 and ok3 and ok4 and ok5
    r, rec2, n2, mk = r.reshape(-1), rec2.reshape(-1), n2.reshape(-1), mk.reshape(-1).view(np.uint8)
    putative = gb.putative_lists(pairs)
    f = rc.FIELD[model]
    changed = 0
    for p, pair in enumerate(pairs):
        rule, refine_rule = rc.rules(model)[0], rc.rules(model)[2]
        ver = rule(putative[p], pair["q_xy"], pair["t_xy"], hc.MAX_ERROR, K, seed + p)
        ref = refine_rule(putative[p], pair["q_xy"], pair["t_xy"], ver, hc.MAX_ERROR, rounds)
        changed += ref["accepted"] > 0
        G = np.asarray(ref[f], np.float32).reshape(3, 3)
        assert r[p]["F"].tobytes() == G.tobytes() and r[p]["inliers"] == ref["inliers"], p
        assert got_acc.reshape(-1)[p] == ref["accepted"], p
        assert mk[up.row0[p]:up.row0[p] + len(putative[p])].tobytes() == ref["mask"].tobytes(), p
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
            fwd, rev = gb.bc.nothing(len(pair["q"])), gb.bc.nothing(len(pair["t"]))
        want2 = cv.filter_matches(*fwd, *rev, img_idx=p)
        assert n2[p] == len(want2) and rec2[up.row0[p]:up.row0[p] + n2[p]].tobytes() == want2.tobytes(), p
    assert changed > 0  # at least one pair's model is the refit: the rematch read refined records
